// The training loader's region-weighted ray sampler on the device (gfx950): GetData.sample_rays
// (NeRFs/HeadNeRF/train/audio_exp_nerf.py:134-195) without a host round trip and without a full-frame ray tensor.
//
//   sample_pixels: per region (face rect minus mouth box | outside the rect | mouth box | torso) the c pixels with the smallest
//                  (Philox key, pixel) pairs, in ascending order -- a uniform c-subset in uniform random order, which is the
//                  distribution of np.random.choice(replace=False), defined so that it can be checked exactly
//                  (include/idealnerf.h: idealnerf_sample_pixels).
//   gather_rays:   the selected pixels' ray origins / directions (the arithmetic of frame_rays_kernel, composite.hip, operation
//                  for operation), ground-truth colours and background colours.
//
// sample_pixels runs ONE workgroup per region (four per launch).  The c-th smallest 64-bit composite (key << 32 | pixel) is found
// by a radix select, 11 bits per pass, with the histogram in LDS; the ten Philox rounds are recomputed in every pass instead of
// storing a key per pixel.  Composites are distinct (the pixel is part of them), so the select is exact, ties of the 32-bit key
// included, and it stops at the first pass whose boundary bin is wholly wanted: two passes for a 450 x 450 frame in practice
// (2^22 key prefixes over 2 x 10^5 pixels), six at most.  The survivors go to LDS in whatever order the lanes arrive, a bitonic
// sort orders them, and the order of arrival is forgotten: the result depends on (map, counts, seed, draw) alone.
#include "march.h"

namespace idn {

constexpr int kSamplerThreads = 1024;
constexpr int kDigitBits = 11;
constexpr int kBins = 1 << kDigitBits;          // 2048 x 4 B of LDS
constexpr int kSelectPasses = 6;                // ceil(64 / 11)
static_assert(kBins == 64 * 32, "find_bin gives every lane of one wave 32 bins");
static_assert(IDN_SAMPLE_MAX_REGION == 4096, "the sort buffer below is 4096 composites = 32 KiB of LDS");

struct SamplerArgs {
    const unsigned char* map;   // [npix] region bits
    int npix;
    int count[4];
    int offset[4];              // first row of each region in sel
    unsigned k0, k1, t0, t1;    // seed and draw, low / high words
    long long* sel;
    int* population;            // [4] workspace: the pixels each region holds, as counted here (-1: count 0, not counted)
};

__device__ __forceinline__ unsigned long long sort_composite(const SamplerArgs& a, unsigned p, unsigned g) {
    unsigned c0 = p, c1 = g, c2 = a.t0, c3 = a.t1;
    philox4x32_10(c0, c1, c2, c3, a.k0, a.k1);
    return ((unsigned long long)c0 << 32) | (unsigned long long)p;
}

// f(p) for every pixel of region g, 16 map bytes per lane and step.  The map may start at any byte address: whole 16-byte
// groups are read with one aligned load, the ragged first and last groups byte by byte inside [0, npix).
template <class F>
__device__ __forceinline__ void for_region_pixels(const SamplerArgs& a, unsigned g, F&& f) {
    const int mis = (int)((unsigned long long)a.map & 15ull);
    const int ngroups = (a.npix + mis + 15) >> 4;
    for (int grp = threadIdx.x; grp < ngroups; grp += kSamplerThreads) {
        const int p0 = grp * 16 - mis;
        unsigned w[4] = {0u, 0u, 0u, 0u};
        if (p0 >= 0 && p0 + 16 <= a.npix) {
            const uint4 v = *reinterpret_cast<const uint4*>(a.map + p0);
            w[0] = v.x; w[1] = v.y; w[2] = v.z; w[3] = v.w;
        } else {
            for (int j = 0; j < 16; ++j) {
                const int p = p0 + j;
                if (p >= 0 && p < a.npix) w[j >> 2] |= (unsigned)a.map[p] << (8 * (j & 3));
            }
        }
        if (((w[0] | w[1] | w[2] | w[3]) & (0x01010101u << g)) == 0u) continue;
#pragma unroll
        for (int j = 0; j < 16; ++j)
            if ((w[j >> 2] >> (8 * (j & 3) + g)) & 1u) f((unsigned)(p0 + j));
    }
}

__global__ __launch_bounds__(kSamplerThreads) void sample_pixels_kernel(SamplerArgs a) {
    __shared__ unsigned hist[kBins];
    __shared__ unsigned long long buf[IDN_SAMPLE_MAX_REGION];
    __shared__ unsigned long long s_prefix;
    __shared__ int s_need, s_done, s_fail, s_n;

    const unsigned g = blockIdx.x;
    const int tid = threadIdx.x;
    const int c = a.count[g];
    long long* out = a.sel + a.offset[g];
    if (c == 0) {
        if (tid == 0) a.population[g] = -1;
        return;
    }
    if (tid == 0) { s_prefix = 0ull; s_need = c; s_done = 0; s_fail = 0; s_n = 0; }

    // ---- radix select of the c-th smallest composite: after pass k the top `decided` bits of it are s_prefix
    int shift = 64;   // composites are compared by v >> shift
    for (int pass = 0; pass < kSelectPasses; ++pass) {
        const int width = min(kDigitBits, shift);
        const int below = shift;          // bits below the already-decided prefix
        shift -= width;
        for (int i = tid; i < kBins; i += kSamplerThreads) hist[i] = 0u;
        __syncthreads();
        const unsigned long long prefix = s_prefix;
        const unsigned mask = (1u << width) - 1u;
        for_region_pixels(a, g, [&](unsigned p) {
            const unsigned long long v = sort_composite(a, p, g);
            if (pass == 0 || (v >> below) == prefix) atomicAdd(&hist[(unsigned)(v >> shift) & mask], 1u);
        });
        __syncthreads();
        if (tid < 64) {   // one wave: lane l sums bins 32 l .. 32 l + 31, a scan finds the lane, the lane finds the bin
            unsigned s = 0u;
            for (int i = 0; i < 32; ++i) s += hist[tid * 32 + i];
            unsigned incl = s;
#pragma unroll
            for (int d = 1; d < 64; d <<= 1) {
                const unsigned o = __shfl_up(incl, d, 64);
                if (tid >= d) incl += o;
            }
            const unsigned total = __shfl(incl, 63, 64);
            const unsigned need = (unsigned)s_need, excl = incl - s;
            if (tid == 0 && pass == 0) a.population[g] = (int)total;
            if (tid == 0 && total < need) s_fail = 1;   // the region holds fewer pixels than asked for
            if (excl < need && need <= incl) {
                unsigned run = excl;
                for (int i = 0; i < 32; ++i) {
                    const unsigned h = hist[tid * 32 + i];
                    if (run + h >= need) {
                        s_prefix = (prefix << width) | (unsigned long long)(tid * 32 + i);
                        s_need = (int)(need - run);
                        s_done = (h == need - run) ? 1 : 0;   // the boundary bin is wanted whole: nothing left to decide
                        break;
                    }
                    run += h;
                }
            }
        }
        __syncthreads();
        if (s_fail || s_done) break;
    }
    if (s_fail) {   // never a partial or repeated pick: the rows say so (the host refuses such counts before any launch)
        for (int i = tid; i < c; i += kSamplerThreads) out[i] = -1;
        return;
    }

    // ---- the c composites at or below the boundary, then in order
    {
        const unsigned long long prefix = s_prefix;
        for_region_pixels(a, g, [&](unsigned p) {
            const unsigned long long v = sort_composite(a, p, g);
            if ((v >> shift) <= prefix) {
                const int at = atomicAdd(&s_n, 1);
                if (at < IDN_SAMPLE_MAX_REGION) buf[at] = v;
            }
        });
    }
    int m = 1;
    while (m < c) m <<= 1;
    __syncthreads();
    for (int i = c + tid; i < m; i += kSamplerThreads) buf[i] = ~0ull;
    __syncthreads();
    for (int k = 2; k <= m; k <<= 1)
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int i = tid; i < m; i += kSamplerThreads) {
                const int l = i ^ j;
                if (l > i) {
                    const unsigned long long x = buf[i], y = buf[l];
                    if ((x > y) == ((i & k) == 0)) { buf[i] = y; buf[l] = x; }
                }
            }
            __syncthreads();
        }
    for (int i = tid; i < c; i += kSamplerThreads) out[i] = (long long)(buf[i] & 0xffffffffull);
}

int launch_sample_pixels(const unsigned char* map, int H, int W, const int counts[4], unsigned long long seed, unsigned long long draw,
                         int* population, long long* sel, hipStream_t s) {
    SamplerArgs a;
    a.map = map;
    a.npix = H * W;
    int off = 0;
    for (int g = 0; g < 4; ++g) {
        a.count[g] = counts[g];
        a.offset[g] = off;
        off += counts[g];
    }
    a.k0 = (unsigned)seed; a.k1 = (unsigned)(seed >> 32);
    a.t0 = (unsigned)draw; a.t1 = (unsigned)(draw >> 32);
    a.sel = sel;
    a.population = population;
    hipLaunchKernelGGL(sample_pixels_kernel, dim3(4), dim3(kSamplerThreads), 0, s, a);
    IDN_HIP_CHECK(hipGetLastError());
    return IDN_OK;
}

// ---------------------------------------------------------------------------
// gather: rays, targets and background of the selected pixels
// ---------------------------------------------------------------------------
struct GatherCam {
    float m[12];
};
// (c2 / batch_rays2: the optional second camera -- the torso stage's frame-0 pose -- for the same pixels; batch_rays2 == nullptr
//  is the one-camera case)
__global__ void gather_rays_kernel(const long long* sel, int n, GatherCam c, GatherCam c2, int W, long npix, float focal, float cx,
                                   float cy, const unsigned char* image, const unsigned char* background, const float* target_table,
                                   const float* background_table, float* batch_rays, float* batch_rays2, float* target_s,
                                   float* bc_rgb) {
    const int idx = blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= n) return;
    const long long pix = sel[idx];
    const bool ok = pix >= 0 && pix < npix;   // a row sample_pixels marked -1 (or a foreign index) reads nothing
    const long q = ok ? (long)pix : 0;
    // from here to d[]: frame_rays_kernel (composite.hip), the same operations in the same order
    const int row = (int)(q / W), col = (int)(q % W);
    const float i = (float)col, j = (float)row;
    const float d0 = (i - cx) / focal;
    const float d1 = -(j - cy) / focal;
    const float d2 = -1.0f;
    auto rays_of = [&](const GatherCam& cam, float* out) {
        float d[3];
#pragma unroll
        for (int r = 0; r < 3; ++r) d[r] = (d0 * cam.m[4 * r + 0] + d1 * cam.m[4 * r + 1]) + d2 * cam.m[4 * r + 2];
#pragma unroll
        for (int r = 0; r < 3; ++r) {
            out[(long)idx * 3 + r] = ok ? cam.m[4 * r + 3] : 0.0f;
            out[((long)n + idx) * 3 + r] = ok ? d[r] : 0.0f;
        }
    };
    rays_of(c, batch_rays);
    if (batch_rays2) rays_of(c2, batch_rays2);
#pragma unroll
    for (int r = 0; r < 3; ++r) {
        target_s[(long)idx * 3 + r] = ok ? target_table[image[q * 3 + r]] : 0.0f;
        bc_rgb[(long)idx * 3 + r] = ok ? background_table[background[q * 3 + r]] : 0.0f;
    }
}

int launch_gather_rays(const long long* sel, int64_t n, const float* c2w_host, const float* c2w2_host, int H, int W, float focal,
                       float cx, float cy, const unsigned char* image, const unsigned char* background, const float* target_table,
                       const float* background_table, float* batch_rays, float* batch_rays2, float* target_s, float* bc_rgb,
                       hipStream_t s) {
    GatherCam c, c2;
    for (int i = 0; i < 12; ++i) c.m[i] = c2w_host[i];
    for (int i = 0; i < 12; ++i) c2.m[i] = c2w2_host ? c2w2_host[i] : 0.0f;
    if (cx < 0) cx = W * 0.5f;
    if (cy < 0) cy = H * 0.5f;
    hipLaunchKernelGGL(gather_rays_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, sel, (int)n, c, c2, W, (long)H * W,
                       focal, cx, cy, image, background, target_table, background_table, batch_rays, c2w2_host ? batch_rays2 : nullptr,
                       target_s, bc_rgb);
    IDN_HIP_CHECK(hipGetLastError());
    return IDN_OK;
}

}  // namespace idn
