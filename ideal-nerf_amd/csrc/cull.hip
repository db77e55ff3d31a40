// Ray cull of the inference frame path (gfx950): an occupancy grid built once per clip from the networks' own sigma, and per
// frame a classification of the pixels into "live" (rendered by the unchanged kernels) and "culled" (every sample has
// sigma_raw <= 0, so raw2outputs gives the background pixel exactly; the value is written down without evaluating a network).
// Memory-light kernels: no MFMA, no atomics, a few hundred bytes of LDS.
//
//   corners  uint8 [(G+1)^3], index ((iz (G+1)) + iy) (G+1) + ix: 1 where the lattice point lo + (ix, iy, iz) cell was marked
//   bits     uint32 [G^3 / 32], word (z G + y) (G / 32) + (x >> 5), bit x & 31: cell (x, y, z) is occupied
//
// Built with -ffp-contract=off like the rest of the library: a pixel's ray comes from frame_ray_dir / frame_ray_record
// (march.h), the functions the frame's own ray kernel calls.
#include "march.h"

namespace idn {

constexpr int kCullThreads = 256;            // four waves per workgroup
constexpr int kCullWaves = kCullThreads / 64;

// ---------------------------------------------------------------------------
// mark: corners[i] |= raw[i].w > sigma_min, one thread per lattice point
// ---------------------------------------------------------------------------
__global__ void cull_mark_kernel(const float4* raw, long n, float sigma_min, unsigned char* corners) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const unsigned char m = raw[i].w > sigma_min ? 1 : 0;
    corners[i] = corners[i] | m;
}

// ---------------------------------------------------------------------------
// cells: one thread computes one whole 32-cell word.  Cell x is occupied when a marked corner lies in a cell within
// Chebyshev distance `dilate` of it: corner indices [x - dilate, x + dilate + 1] on each axis, clamped to the lattice.
// ---------------------------------------------------------------------------
__global__ void cull_cells_kernel(const unsigned char* corners, int G, int dilate, unsigned* bits) {
    const int wpr = G >> 5;
    const long n_words = (long)G * G * wpr;
    const long w = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (w >= n_words) return;
    const int xw = (int)(w % wpr), y = (int)((w / wpr) % G), z = (int)(w / ((long)wpr * G));
    const int C = G + 1, x0 = xw * 32;
    const int z_lo = max(z - dilate, 0), z_hi = min(z + dilate + 1, G);
    const int y_lo = max(y - dilate, 0), y_hi = min(y + dilate + 1, G);
    const int c_lo = max(x0 - dilate, 0), c_hi = min(x0 + 31 + dilate + 1, G);
    unsigned word = 0u;
    for (int cx = c_lo; cx <= c_hi; ++cx) {
        bool any = false;
        for (int cz = z_lo; cz <= z_hi && !any; ++cz)
            for (int cy = y_lo; cy <= y_hi && !any; ++cy) any = corners[((long)cz * C + cy) * C + cx] != 0;
        if (!any) continue;
        // the cells x of this word with cx in [x - dilate, x + dilate + 1]
        const int b_lo = max(cx - dilate - 1 - x0, 0), b_hi = min(cx + dilate - x0, 31);
        if (b_lo > b_hi) continue;
        const unsigned upto_hi = b_hi == 31 ? 0xffffffffu : ((1u << (b_hi + 1)) - 1u);
        word |= upto_hi & ~((1u << b_lo) - 1u);
    }
    bits[w] = word;
}

// ---------------------------------------------------------------------------
// classify + compact: three launches, no atomics, the order of `sel` is the pixel order whatever the scheduling
//   1 count : one thread per pixel marches its ray; a wave's ballot goes to masks[], a workgroup's count to counts[]
//   2 scan  : ONE workgroup turns counts[] into exclusive offsets in index order and writes n_live
//   3 write : every live pixel's slot = its workgroup's offset + the live pixels before it in the workgroup (ballots)
// ---------------------------------------------------------------------------
struct CullGridDev {
    const unsigned* bits;
    int G;
    float lo[3];
    float cell;
};
struct CullFrameDev {
    C2W c;
    int W;
    float focal, cx, cy, near_, far_;
    long pix0;   // first pixel of the row band (row-major index in the frame)
    int npix;    // pixels of the band
};

// a march point outside the box was never evaluated when the grid was built: it counts as occupied
__device__ __forceinline__ bool cull_point_occupied(const CullGridDev& g, float px, float py, float pz) {
    const float tx = (px - g.lo[0]) / g.cell, ty = (py - g.lo[1]) / g.cell, tz = (pz - g.lo[2]) / g.cell;
    const float Gf = (float)g.G;
    if (!(tx >= 0.0f && tx < Gf && ty >= 0.0f && ty < Gf && tz >= 0.0f && tz < Gf)) return true;   // (a NaN lands here too)
    const int x = (int)tx, y = (int)ty, z = (int)tz;   // in [0, G): truncation is floor
    const unsigned word = g.bits[((long)z * g.G + y) * (g.G >> 5) + (x >> 5)];
    return (word >> (x & 31)) & 1u;
}

__global__ void __launch_bounds__(kCullThreads) cull_count_kernel(CullGridDev g, CullFrameDev f, float dz, int K,
                                                                   unsigned long long* masks, int* counts) {
    __shared__ int wave_count[kCullWaves];
    const int idx = blockIdx.x * kCullThreads + threadIdx.x;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    bool live = false;
    if (idx < f.npix) {
        float d[3];
        frame_ray_dir(f.c, f.W, f.focal, f.cx, f.cy, f.pix0 + idx, d);
        const float ox = f.c.m[3], oy = f.c.m[7], oz = f.c.m[11];
        for (int k = 0; k <= K && !live; ++k) {
            const float z = k == K ? f.far_ : f.near_ + (float)k * dz;
            live = cull_point_occupied(g, ox + d[0] * z, oy + d[1] * z, oz + d[2] * z);
        }
    }
    const unsigned long long ballot = __ballot(live);
    if (lane == 0) {
        masks[(long)blockIdx.x * kCullWaves + wave] = ballot;
        wave_count[wave] = __popcll(ballot);
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        int c = 0;
#pragma unroll
        for (int i = 0; i < kCullWaves; ++i) c += wave_count[i];
        counts[blockIdx.x] = c;
    }
}

__global__ void __launch_bounds__(kCullThreads) cull_scan_kernel(const int* counts, int n_blocks, int* offsets, int* n_live) {
    __shared__ int wave_total[kCullWaves];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int carry = 0;   // live pixels of the workgroups before this chunk (the same value in every thread)
    for (int base = 0; base < n_blocks; base += kCullThreads) {
        const int i = base + threadIdx.x;
        const int c = i < n_blocks ? counts[i] : 0;
        int incl = c;   // inclusive scan across the wave
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const int o = __shfl_up(incl, d, 64);
            if (lane >= d) incl += o;
        }
        if (lane == 63) wave_total[wave] = incl;
        __syncthreads();
        int before = 0, total = 0;
#pragma unroll
        for (int w = 0; w < kCullWaves; ++w) {
            if (w < wave) before += wave_total[w];
            total += wave_total[w];
        }
        if (i < n_blocks) offsets[i] = carry + before + incl - c;
        carry += total;
        __syncthreads();   // wave_total is rewritten by the next chunk
    }
    if (threadIdx.x == 0) *n_live = carry;
}

__global__ void __launch_bounds__(kCullThreads) cull_write_kernel(const unsigned long long* masks, const int* offsets, int npix,
                                                                   long long* sel) {
    const int idx = blockIdx.x * kCullThreads + threadIdx.x;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const unsigned long long* m = masks + (long)blockIdx.x * kCullWaves;
    int pos = offsets[blockIdx.x];
    for (int w = 0; w < wave; ++w) pos += __popcll(m[w]);
    const unsigned long long mine = m[wave];
    if (idx < npix && ((mine >> lane) & 1ull)) {
        pos += __popcll(mine & ((1ull << lane) - 1ull));
        sel[pos] = (long long)idx;   // pos < n_live <= npix, and pos grows with idx: sel is ascending
    }
}

size_t cull_classify_workspace_bytes(int64_t npix) {
    const size_t n_blocks = (size_t)((npix + kCullThreads - 1) / kCullThreads);
    return n_blocks * (kCullWaves * sizeof(unsigned long long) + 2 * sizeof(int));
}

static void frame_dev(const idn_frame& f, CullFrameDev* o) {
    for (int i = 0; i < 12; ++i) o->c.m[i] = f.c2w[i];
    o->W = f.W;
    o->focal = f.focal;
    o->cx = f.cx < 0 ? f.W * 0.5f : f.cx;
    o->cy = f.cy < 0 ? f.H * 0.5f : f.cy;
    o->near_ = f.near_;
    o->far_ = f.far_;
    o->pix0 = (long)f.row0 * f.W;
    o->npix = f.nrows * f.W;
}

int launch_cull_mark(const float* raw, int64_t n, float sigma_min, unsigned char* corners, hipStream_t s) {
    hipLaunchKernelGGL(cull_mark_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, (const float4*)raw, (long)n, sigma_min,
                       corners);
    IDN_HIP_CHECK(hipGetLastError());
    return IDN_OK;
}

int launch_cull_cells(const unsigned char* corners, int G, int dilate, unsigned* bits, hipStream_t s) {
    const long n_words = (long)G * G * (G >> 5);
    hipLaunchKernelGGL(cull_cells_kernel, dim3((unsigned)((n_words + 255) / 256)), dim3(256), 0, s, corners, G, dilate, bits);
    IDN_HIP_CHECK(hipGetLastError());
    return IDN_OK;
}

int launch_cull_classify(const idn_cull_grid& grid, const idn_frame& frame, float dz, int K, long long* sel, int* n_live, void* ws,
                         hipStream_t s) {
    CullGridDev g;
    g.bits = grid.bits;
    g.G = grid.G;
    for (int i = 0; i < 3; ++i) g.lo[i] = grid.lo[i];
    g.cell = grid.cell;
    CullFrameDev f;
    frame_dev(frame, &f);
    const int n_blocks = (f.npix + kCullThreads - 1) / kCullThreads;
    unsigned long long* masks = (unsigned long long*)ws;
    int* counts = (int*)(masks + (size_t)n_blocks * kCullWaves);
    int* offsets = counts + n_blocks;
    hipLaunchKernelGGL(cull_count_kernel, dim3(n_blocks), dim3(kCullThreads), 0, s, g, f, dz, K, masks, counts);
    IDN_HIP_CHECK(hipGetLastError());
    hipLaunchKernelGGL(cull_scan_kernel, dim3(1), dim3(kCullThreads), 0, s, (const int*)counts, n_blocks, offsets, n_live);
    IDN_HIP_CHECK(hipGetLastError());
    hipLaunchKernelGGL(cull_write_kernel, dim3(n_blocks), dim3(kCullThreads), 0, s, (const unsigned long long*)masks,
                       (const int*)offsets, f.npix, sel);
    IDN_HIP_CHECK(hipGetLastError());
    return IDN_OK;
}

// ---------------------------------------------------------------------------
// sample cull: the same count / scan / write over the points P = ray S + s of a depth array z [n, S].  A point is SKIPPABLE
// when its cell is clear and raw2outputs cannot tell its network output from (0, 0, 0, 0): it is its ray's last sample (the
// colour is replaced by the background pixel, and sigma_raw <= 0 gives the alpha of sigma_raw = 0), or the spacing to the
// next sample is so short that alpha is +0.0f (the colour gate's fact, mlp_common.h: gate_point_dead).  Every other point
// is LIVE; so is one with a NaN in its position (cull_point_occupied) or its spacing (the comparison is false).
// ---------------------------------------------------------------------------
// the point as point_of<kModeRays> forms it (mlp_common.h): product and sum rounded separately
__device__ __forceinline__ void cull_sample_point(const float* rr, float z, float (&p)[3]) {
    p[0] = rr[0] + rr[3] * z;
    p[1] = rr[1] + rr[4] * z;
    p[2] = rr[2] + rr[5] * z;
}

__global__ void __launch_bounds__(kCullThreads) cull_sample_count_kernel(CullGridDev g, const float* rays, const float* z, int S,
                                                                          long n_points, unsigned long long* masks, int* counts) {
    __shared__ int wave_count[kCullWaves];
    const long P = (long)blockIdx.x * kCullThreads + threadIdx.x;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    bool live = false;
    if (P < n_points) {
        const unsigned ray = (unsigned)P / (unsigned)S;   // n_points < 2^31 (checked by the entry)
        const bool last = (unsigned)P - ray * (unsigned)S == (unsigned)S - 1u;
        const float* rr = rays + (long)ray * IDN_RAY_FLOATS;
        const float zc = z[P], zn = z[last ? P : P + 1];   // never past a ray's (and so the array's) end
        float p[3];
        cull_sample_point(rr, zc, p);
        // dist of composite_ray (march.h) and gate_point_dead, same operations in the same order
        const float dn = sqrtf((rr[3] * rr[3] + rr[4] * rr[4]) + rr[5] * rr[5]);
        float dist = zn - zc;
        dist = dist * dn;
        const bool skippable = !cull_point_occupied(g, p[0], p[1], p[2]) && (last || fabsf(dist) <= kGateMaxDist);
        live = !skippable;
    }
    const unsigned long long ballot = __ballot(live);
    if (lane == 0) {
        masks[(long)blockIdx.x * kCullWaves + wave] = ballot;
        wave_count[wave] = __popcll(ballot);
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        int c = 0;
#pragma unroll
        for (int i = 0; i < kCullWaves; ++i) c += wave_count[i];
        counts[blockIdx.x] = c;
    }
}

int launch_cull_sample_classify(const idn_cull_grid& grid, const float* rays, const float* z, int64_t n_points, int S, long long* sel,
                                int* n_live, void* ws, hipStream_t s) {
    CullGridDev g;
    g.bits = grid.bits;
    g.G = grid.G;
    for (int i = 0; i < 3; ++i) g.lo[i] = grid.lo[i];
    g.cell = grid.cell;
    const int n_blocks = (int)((n_points + kCullThreads - 1) / kCullThreads);
    unsigned long long* masks = (unsigned long long*)ws;
    int* counts = (int*)(masks + (size_t)n_blocks * kCullWaves);
    int* offsets = counts + n_blocks;
    hipLaunchKernelGGL(cull_sample_count_kernel, dim3(n_blocks), dim3(kCullThreads), 0, s, g, rays, z, S, (long)n_points, masks, counts);
    IDN_HIP_CHECK(hipGetLastError());
    hipLaunchKernelGGL(cull_scan_kernel, dim3(1), dim3(kCullThreads), 0, s, (const int*)counts, n_blocks, offsets, n_live);
    IDN_HIP_CHECK(hipGetLastError());
    hipLaunchKernelGGL(cull_write_kernel, dim3(n_blocks), dim3(kCullThreads), 0, s, (const unsigned long long*)masks,
                       (const int*)offsets, (int)n_points, sel);
    IDN_HIP_CHECK(hipGetLastError());
    return IDN_OK;
}

// pts[j] = the point sel[j] (recomputed as above), dirs[j] = its ray's view direction: idealnerf_query_points_fwd's inputs, S = 1
__global__ void cull_sample_gather_kernel(const long long* sel, long m, const float* rays, const float* z, int S, long n_points,
                                          float* pts, float* dirs) {
    const long j = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= m) return;
    const long long P0 = sel[j];
    const long P = (P0 >= 0 && P0 < n_points) ? (long)P0 : 0;   // a foreign index reads nothing outside the arrays
    const float* rr = rays + (P / S) * IDN_RAY_FLOATS;
    float p[3];
    cull_sample_point(rr, z[P], p);
#pragma unroll
    for (int r = 0; r < 3; ++r) {
        pts[j * 3 + r] = p[r];
        dirs[j * 3 + r] = rr[8 + r];
    }
}

int launch_cull_sample_gather(const long long* sel, int64_t m, const float* rays, const float* z, int64_t n_points, int S, float* pts,
                              float* dirs, hipStream_t s) {
    hipLaunchKernelGGL(cull_sample_gather_kernel, dim3((unsigned)((m + 255) / 256)), dim3(256), 0, s, sel, (long)m, rays, z, S,
                       (long)n_points, pts, dirs);
    IDN_HIP_CHECK(hipGetLastError());
    return IDN_OK;
}

// raw [n_points, 4]: +0.0f everywhere (a fill), then raw_live[j] at sel[j]; sel holds each point once, so no two threads
// write one address and the bytes are the same on every run
__global__ void cull_sample_scatter_kernel(const long long* sel, long m, const float4* raw_live, long n_points, float4* raw) {
    const long j = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= m) return;
    const long long P = sel[j];
    if (P < 0 || P >= n_points) return;   // a foreign index writes nothing
    raw[P] = raw_live[j];
}

int launch_cull_sample_scatter(const long long* sel, int64_t m, const float* raw_live, int64_t n_points, float* raw, hipStream_t s) {
    IDN_HIP_CHECK(hipMemsetAsync(raw, 0, (size_t)n_points * 4 * sizeof(float), s));
    if (m > 0) {
        hipLaunchKernelGGL(cull_sample_scatter_kernel, dim3((unsigned)((m + 255) / 256)), dim3(256), 0, s, sel, (long)m,
                           (const float4*)raw_live, (long)n_points, (float4*)raw);
        IDN_HIP_CHECK(hipGetLastError());
    }
    return IDN_OK;
}

// ---------------------------------------------------------------------------
// gather: the ray records and background pixels of the live pixels, in the order of `sel`
// ---------------------------------------------------------------------------
__global__ void cull_gather_kernel(const long long* sel, int n, CullFrameDev f, const float* bc, float* rays, float* bc_live) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const long long q0 = sel[i];
    const bool ok = q0 >= 0 && q0 < f.npix;   // a foreign index reads nothing outside the band
    const long q = ok ? (long)q0 : 0;
    frame_ray_record(f.c, f.W, f.focal, f.cx, f.cy, f.near_, f.far_, f.pix0 + q, rays + (long)i * IDN_RAY_FLOATS);
#pragma unroll
    for (int r = 0; r < 3; ++r) bc_live[(long)i * 3 + r] = bc[q * 3 + r];
}

int launch_cull_gather(const long long* sel, int64_t n, const idn_frame& frame, const float* bc, float* rays, float* bc_live,
                       hipStream_t s) {
    CullFrameDev f;
    frame_dev(frame, &f);
    hipLaunchKernelGGL(cull_gather_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, sel, (int)n, f, bc, rays, bc_live);
    IDN_HIP_CHECK(hipGetLastError());
    return IDN_OK;
}

// ---------------------------------------------------------------------------
// fill + scatter: every pixel's culled value, then the live rows over them (two launches on one stream)
// ---------------------------------------------------------------------------
struct CullOutputs {
    idn_cull_output o[IDN_CULL_MAX_OUTPUTS];
    int n;
};

__global__ void cull_fill_kernel(CullOutputs outs, const float* bc, long npix) {
    const long q = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= npix) return;
    for (int k = 0; k < outs.n; ++k) {
        const idn_cull_output& o = outs.o[k];
        for (int c = 0; c < o.channels; ++c) o.dense[q * o.channels + c] = o.fill_background ? bc[q * 3 + c] : o.value;
    }
}

__global__ void cull_scatter_kernel(CullOutputs outs, const long long* sel, long n_live, long npix) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_live) return;
    const long long q = sel[i];
    if (q < 0 || q >= npix) return;   // a foreign index writes nothing
    for (int k = 0; k < outs.n; ++k) {
        const idn_cull_output& o = outs.o[k];
        for (int c = 0; c < o.channels; ++c) o.dense[q * o.channels + c] = o.live[i * o.channels + c];
    }
}

int launch_cull_scatter(const long long* sel, int64_t n_live, int64_t npix, const float* bc, const idn_cull_output* outs, int n_outs,
                        hipStream_t s) {
    CullOutputs o;
    o.n = n_outs;
    for (int k = 0; k < n_outs; ++k) o.o[k] = outs[k];
    hipLaunchKernelGGL(cull_fill_kernel, dim3((unsigned)((npix + 255) / 256)), dim3(256), 0, s, o, bc, (long)npix);
    IDN_HIP_CHECK(hipGetLastError());
    if (n_live > 0) {
        hipLaunchKernelGGL(cull_scatter_kernel, dim3((unsigned)((n_live + 255) / 256)), dim3(256), 0, s, o, sel, (long)n_live,
                           (long)npix);
        IDN_HIP_CHECK(hipGetLastError());
    }
    return IDN_OK;
}

}  // namespace idn
