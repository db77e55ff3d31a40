// Per-ray stages around the MLP (gfx950): ray generation, coarse depths, alpha
// compositing, inverse-CDF importance sampling + merge.  One 64-lane wavefront per ray;
// prefix products / sums are wave-level scans in fp64 (PyTorch-CPU's cumprod / cumsum
// accumulate in double and round each output to fp32 -- DESIGN.md "numerics").
//
// Built with -ffp-contract=off: every product and sum below rounds separately, as the
// reference's chain of eager ops does; the sample positions feed index decisions.
#include "march.h"

namespace idn {

// ---------------------------------------------------------------------------
// a1: get_rays + record assembly (helper.py:228-243, audio_exp_nerf.py:396-427)
// ---------------------------------------------------------------------------
__global__ void frame_rays_kernel(C2W c, int W, float focal, float cx, float cy, float near_, float far_, long pix0,
                                  int npix, float* out) {
    const int idx = blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= npix) return;
    frame_ray_record(c, W, focal, cx, cy, near_, far_, pix0 + idx, out + (long)idx * IDN_RAY_FLOATS);
}

// the records of the pixels [pix0, pix0 + npix) of the frame (row-major): a band of whole rows, or one pass of a frame-mode render
int launch_frame_rays_pixels(const float* c2w_host, int H, int W, float focal, float cx, float cy, float near_, float far_,
                             int64_t pix0, int npix, float* rays_out, hipStream_t s) {
    C2W c;
    for (int i = 0; i < 12; ++i) c.m[i] = c2w_host[i];
    if (cx < 0) cx = W * 0.5f;
    if (cy < 0) cy = H * 0.5f;
    if (npix <= 0) return IDN_OK;
    hipLaunchKernelGGL(frame_rays_kernel, dim3((npix + 255) / 256), dim3(256), 0, s, c, W, focal, cx, cy, near_, far_,
                       (long)pix0, npix, rays_out);
    IDN_HIP_CHECK(hipGetLastError());
    return IDN_OK;
}

// ---------------------------------------------------------------------------
// a3: coarse depths (audio_exp_nerf.py:306-330)
// ---------------------------------------------------------------------------
__global__ void coarse_depths_kernel(const float* rays, const float* t_vals, const float* t_rand, long n_rays, int S,
                                     int lindisp, float* z, Draws draws) {
    const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= n_rays * S) return;
    const long r = idx / S;
    const int s = (int)(idx - r * S);
    const float near_ = rays[r * IDN_RAY_FLOATS + 6], far_ = rays[r * IDN_RAY_FLOATS + 7];
    auto zlin = [&](int k) {
        const float t = t_vals[k];
        if (lindisp) return 1.0f / (1.0f / near_ * (1.0f - t) + 1.0f / far_ * t);   // linear in inverse depth (:309-310)
        return near_ * (1.0f - t) + far_ * t;
    };
    float zz = zlin(s);
    if (t_rand || draws.on) {
        const float lower = (s == 0) ? zz : 0.5f * (zz + zlin(s - 1));
        const float upper = (s == S - 1) ? zz : 0.5f * (zlin(s + 1) + zz);
        const float tr = (s == S - 1) ? 1.0f : draws.on ? draw_t_rand(draws, r, s) : t_rand[idx];
        zz = lower + (upper - lower) * tr;
    }
    z[idx] = zz;
}

int launch_coarse_depths(const float* rays, const float* t_vals, const float* t_rand, int64_t n_rays, int S,
                         int lindisp, float* z, Draws draws, hipStream_t s) {
    const long total = (long)n_rays * S;
    if (total <= 0) return IDN_OK;
    hipLaunchKernelGGL(coarse_depths_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, rays, t_vals,
                       t_rand, (long)n_rays, S, lindisp, z, draws);
    IDN_HIP_CHECK(hipGetLastError());
    return IDN_OK;
}

// The table the in-kernel draws come from, as a tensor (include/idealnerf.h: idealnerf_philox_uniform)
__global__ void philox_uniform_kernel(unsigned long long seed, int which, long row0, long n_rows, int n_cols, float* out) {
    const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= n_rows * n_cols) return;
    const long r = idx / n_cols;
    const int c = (int)(idx - r * n_cols);
    out[idx] = philox_uniform(seed, 2ull * (unsigned long long)(row0 + r) + (unsigned long long)which, (unsigned)c);
}
int launch_philox_uniform(unsigned long long seed, int which, int64_t row0, int64_t n_rows, int n_cols, float* out, hipStream_t s) {
    const long total = (long)n_rows * n_cols;
    if (total <= 0) return IDN_OK;
    hipLaunchKernelGGL(philox_uniform_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, seed, which, (long)row0, (long)n_rows, n_cols, out);
    IDN_HIP_CHECK(hipGetLastError());
    return IDN_OK;
}

// ---------------------------------------------------------------------------
// frame tail: to8b (NeRFs/HeadNeRF/helper.py:154, `(255 * np.clip(x, 0, 1)).astype(np.uint8)`) and
// the NaN/Inf scan of the render dict (audio_exp_nerf.py:367-369) as ONE device-side flag.
// 255 * clip(x) is an fp32 product, astype truncates.  A NaN pixel is written as 0 and flagged.
// ---------------------------------------------------------------------------
__global__ void to8b_kernel(const float* __restrict__ rgb, long n_values, int swap_rb, unsigned char* __restrict__ out,
                            int* __restrict__ flag) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    bool bad = false;
    if (i < n_values) {
        const float x = rgb[i];
        bad = !(fabsf(x) <= 3.402823466e+38f);  // NaN or +-Inf
        float c = x < 0.0f ? 0.0f : (x > 1.0f ? 1.0f : x);
        if (x != x) c = 0.0f;
        const long px = i / 3;
        const int ch = (int)(i - px * 3);
        out[px * 3 + (swap_rb ? 2 - ch : ch)] = (unsigned char)(int)(255.0f * c);
    }
    if (flag && __any(bad) && (threadIdx.x & 63) == 0) atomicOr(flag, 1);
}

int launch_to8b(const float* rgb, int64_t n_pixels, int swap_rb, unsigned char* out, int* flag, hipStream_t s) {
    const long n = (long)n_pixels * 3;
    if (n <= 0) return IDN_OK;
    hipLaunchKernelGGL(to8b_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, rgb, n, swap_rb, out, flag);
    IDN_HIP_CHECK(hipGetLastError());
    return IDN_OK;
}

// ---------------------------------------------------------------------------
// clip tail of the head + torso flow (NeRFs/TorsoNeRF/test_torso.py:523-525):
//   out = to8b(rgb_head * last_weight[:, None] + rgb_fg),   fg_out = to8b(rgb_fg) (optional)
// One pass over 28 B/pixel instead of a multiply, an add and to8b with two full-frame temporaries.
// The product and the sum are separate fp32 operations (this file is built with -ffp-contract=off),
// so a finite composite gives the bytes of to8b on the eager expression.  A non-finite composite is
// written as 0 and flagged; any NaN/Inf input makes the composite non-finite, so no input scan is needed.
// ---------------------------------------------------------------------------
__device__ __forceinline__ unsigned to8b_value(float x) {   // to8b_kernel's arithmetic for one value
    float c = x < 0.0f ? 0.0f : (x > 1.0f ? 1.0f : x);
    if (x != x) c = 0.0f;
    return (unsigned)(int)(255.0f * c);
}
__device__ __forceinline__ unsigned compose_value(float head, float w, float fg, bool& bad) {
    const float p = head * w;
    const float x = p + fg;
    const bool nf = !(fabsf(x) <= 3.402823466e+38f);
    bad |= nf;
    return nf ? 0u : to8b_value(x);
}

// VEC: thread t owns pixels 4t .. 4t+3 = floats 12t .. 12t+11 of each RGB stream (three float4), one float4 of weights
// and bytes 12t .. 12t+11 of each output (three dwords; 12t is 4-byte aligned whenever the base is).  !VEC: one pixel
// per thread, starting at pixel `first` (the n % 4 tail, or everything when a base pointer is not 16-byte aligned).
template <bool VEC, bool FG>
__global__ __launch_bounds__(256) void compose_to8b_kernel(const float* __restrict__ head, const float* __restrict__ lw,
                                                           const float* __restrict__ fg, long first, long count, int swap_rb,
                                                           unsigned char* __restrict__ out, unsigned char* __restrict__ fg_out,
                                                           int* __restrict__ flag) {
    const long t = (long)blockIdx.x * blockDim.x + threadIdx.x;
    bool bad = false;
    if (t < count) {
        if constexpr (VEC) {
            const float4* h4 = reinterpret_cast<const float4*>(head) + 3 * t;
            const float4* f4 = reinterpret_cast<const float4*>(fg) + 3 * t;
            const float4 w4 = reinterpret_cast<const float4*>(lw)[t];
            const float4 ha = h4[0], hb = h4[1], hc = h4[2];
            const float4 fa = f4[0], fb = f4[1], fc = f4[2];
            const float h[12] = {ha.x, ha.y, ha.z, ha.w, hb.x, hb.y, hb.z, hb.w, hc.x, hc.y, hc.z, hc.w};
            const float f[12] = {fa.x, fa.y, fa.z, fa.w, fb.x, fb.y, fb.z, fb.w, fc.x, fc.y, fc.z, fc.w};
            const float w[4] = {w4.x, w4.y, w4.z, w4.w};
            unsigned b[12], g[12];
#pragma unroll
            for (int p = 0; p < 4; ++p) {
#pragma unroll
                for (int c = 0; c < 3; ++c) {
                    b[3 * p + c] = compose_value(h[3 * p + c], w[p], f[3 * p + c], bad);
                    if constexpr (FG) g[3 * p + c] = to8b_value(f[3 * p + c]);
                }
                if (swap_rb) {   // selects on constant register indices, no indexed register array
                    const unsigned r = b[3 * p];
                    b[3 * p] = b[3 * p + 2];
                    b[3 * p + 2] = r;
                    if constexpr (FG) {
                        const unsigned q = g[3 * p];
                        g[3 * p] = g[3 * p + 2];
                        g[3 * p + 2] = q;
                    }
                }
            }
            unsigned* o = reinterpret_cast<unsigned*>(out) + 3 * t;
#pragma unroll
            for (int d = 0; d < 3; ++d) o[d] = b[4 * d] | (b[4 * d + 1] << 8) | (b[4 * d + 2] << 16) | (b[4 * d + 3] << 24);
            if constexpr (FG) {
                unsigned* og = reinterpret_cast<unsigned*>(fg_out) + 3 * t;
#pragma unroll
                for (int d = 0; d < 3; ++d) og[d] = g[4 * d] | (g[4 * d + 1] << 8) | (g[4 * d + 2] << 16) | (g[4 * d + 3] << 24);
            }
        } else {
            const long px = first + t;
            const float w = lw[px];
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const long dst = px * 3 + (swap_rb ? 2 - c : c);
                out[dst] = (unsigned char)compose_value(head[px * 3 + c], w, fg[px * 3 + c], bad);
                if constexpr (FG) fg_out[dst] = (unsigned char)to8b_value(fg[px * 3 + c]);
            }
        }
    }
    if (flag && __any(bad) && (threadIdx.x & 63) == 0) atomicOr(flag, 1);
}

int launch_compose_to8b(const float* head, const float* lw, const float* fg, int64_t n_pixels, int swap_rb,
                        unsigned char* out, unsigned char* fg_out, int* flag, hipStream_t s) {
    if (n_pixels <= 0) return IDN_OK;
    const uintptr_t in_bits = (uintptr_t)head | (uintptr_t)lw | (uintptr_t)fg;
    const uintptr_t out_bits = (uintptr_t)out | (uintptr_t)fg_out;   // fg_out == NULL adds no bits
    const bool aligned = (in_bits & 15) == 0 && (out_bits & 3) == 0;
    const long quads = aligned ? (long)(n_pixels / 4) : 0;
    const long first = quads * 4, rest = (long)n_pixels - first;
    const dim3 block(256);
    if (quads > 0) {
        const dim3 grid((unsigned)((quads + 255) / 256));
        if (fg_out) hipLaunchKernelGGL((compose_to8b_kernel<true, true>), grid, block, 0, s, head, lw, fg, 0L, quads, swap_rb, out, fg_out, flag);
        else hipLaunchKernelGGL((compose_to8b_kernel<true, false>), grid, block, 0, s, head, lw, fg, 0L, quads, swap_rb, out, fg_out, flag);
        IDN_HIP_CHECK(hipGetLastError());
    }
    if (rest > 0) {
        const dim3 grid((unsigned)((rest + 255) / 256));
        if (fg_out) hipLaunchKernelGGL((compose_to8b_kernel<false, true>), grid, block, 0, s, head, lw, fg, first, rest, swap_rb, out, fg_out, flag);
        else hipLaunchKernelGGL((compose_to8b_kernel<false, false>), grid, block, 0, s, head, lw, fg, first, rest, swap_rb, out, fg_out, flag);
        IDN_HIP_CHECK(hipGetLastError());
    }
    return IDN_OK;
}

template <int SPL>
__global__ __launch_bounds__(256) void composite_kernel(const float4* raw, const float* z, const float* rays,
                                                        const float* bc, long n_rays, int S, const float* noise,
                                                        int white_bkgd, idn_composite_out out) {
    const int lane = threadIdx.x & 63;
    const long ray = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (ray >= n_rays) return;  // wave-uniform
    float w[SPL];
    composite_ray<SPL>(raw + ray * S, z + ray * S, rays, bc, ray, lane, S, noise, white_bkgd, out, w);
}

// f(std::integral_constant<int, SPL>{}), SPL = min(spl, MAX) samples per lane (counting down emits the kernels in the order 1..MAX)
template <int MAX, class F>
static void dispatch_spl(int spl, F&& f) {
    if constexpr (MAX > 1)
        if (spl < MAX) return dispatch_spl<MAX - 1>(spl, f);
    f(std::integral_constant<int, MAX>{});
}

int launch_composite(const CompositeIn& in, const idn_composite_out& out, hipStream_t s) {
    if (in.n_rays <= 0) return IDN_OK;
    if (in.S < 2 || in.S > 64 * kMaxSpl) return fail(IDN_EUNSUPPORTED, "composite: n_samples %d outside [2, %d]", in.S, 64 * kMaxSpl);
    dispatch_spl<kMaxSpl>((in.S + 63) / 64, [&](auto spl) {
        hipLaunchKernelGGL(composite_kernel<decltype(spl)::value>, dim3((unsigned)((in.n_rays + 3) / 4)), dim3(256), 0, s,
                           reinterpret_cast<const float4*>(in.raw), in.z, in.rays, in.bc, (long)in.n_rays, in.S, in.noise, in.white_bkgd, out);
    });
    IDN_HIP_CHECK(hipGetLastError());
    return IDN_OK;
}

__global__ __launch_bounds__(256) void sample_pdf_kernel(SampleArgs a) {
    __shared__ float s_cdf[4][kMaxBins];
    __shared__ float s_bins[4][kMaxBins];
    __shared__ float s_val[4][kMaxFine];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const long ray = (long)blockIdx.x * 4 + wv;
    if (ray >= a.n_rays) return;  // wave-uniform; no block-level barrier below
    sample_pdf_ray(a, ray, lane, s_cdf[wv], s_bins[wv], s_val[wv], nullptr);
}

// ---------------------------------------------------------------------------
// The ray march between the two network passes as ONE kernel (audio_exp_nerf.py:335-349): coarse
// raw2outputs, sample_pdf and the sorted merge, one wave per ray.  The compositing weights go from the
// lanes' registers into the wave's LDS row and the pdf / cdf / inversion / merge run on them there: the
// [n, S] weight matrix never exists in HBM (unless its debug tap is asked for), and the coarse pass of a
// render is MLP -> march -> MLP -> composite.
// ---------------------------------------------------------------------------
template <int SPL>
__global__ __launch_bounds__(256) void march_kernel(const float4* raw, const float* rays, const float* bc, const float* noise,
                                                    int white_bkgd, idn_composite_out out, SampleArgs a) {
    __shared__ float s_cdf[4][kMaxBins];
    __shared__ float s_bins[4][kMaxBins];
    __shared__ float s_val[4][kMaxFine];
    __shared__ float s_w[4][kMaxBins + 1];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const long ray = (long)blockIdx.x * 4 + wv;
    if (ray >= a.n_rays) return;  // wave-uniform; no block-level barrier below
    float w[SPL];
    composite_ray<SPL>(raw + ray * a.S, a.z + ray * a.S, rays, bc, ray, lane, a.S, noise, white_bkgd, out, w);
#pragma unroll
    for (int i = 0; i < SPL; ++i)
        if (lane * SPL + i < a.S) s_w[wv][lane * SPL + i] = w[i];
    wave_lds_fence();
    sample_pdf_ray(a, ray, lane, s_cdf[wv], s_bins[wv], s_val[wv], s_w[wv]);
}

int launch_march(const CompositeIn& in, const idn_composite_out& out, const SampleArgs& a, hipStream_t s) {
    if (a.n_rays <= 0) return IDN_OK;
    const int S = a.S, Ni = a.Ni;
    if (S < 3 || S > 64 * kMaxSpl || a.nb > kMaxBins - 1) return fail(IDN_EUNSUPPORTED, "march: n_samples %d outside [3, %d]", S, kMaxBins);
    if (Ni < 1 || Ni > kMaxNi) return fail(IDN_EUNSUPPORTED, "march: n_importance %d outside [1, %d]", Ni, kMaxNi);
    if (S + Ni > kMaxFine) return fail(IDN_EUNSUPPORTED, "march: n_samples + n_importance > %d", kMaxFine);
    dispatch_spl<4>((S + 63) / 64, [&](auto spl) {
        hipLaunchKernelGGL(march_kernel<decltype(spl)::value>, dim3((unsigned)((a.n_rays + 3) / 4)), dim3(256), 0, s,
                           reinterpret_cast<const float4*>(in.raw), in.rays, in.bc, in.noise, in.white_bkgd, out, a);
    });
    IDN_HIP_CHECK(hipGetLastError());
    return IDN_OK;
}

int launch_sample_pdf(const SampleArgs& a, hipStream_t s) {
    if (a.n_rays <= 0) return IDN_OK;
    if (a.nb < 2 || a.nb > kMaxBins - 1) return fail(IDN_EUNSUPPORTED, "sample_pdf: %d bins outside [2, %d]", a.nb, kMaxBins - 1);
    if (a.Ni < 1 || a.Ni > kMaxNi) return fail(IDN_EUNSUPPORTED, "sample_pdf: n_importance %d outside [1, %d]", a.Ni, kMaxNi);
    if (a.S + a.Ni > kMaxFine) return fail(IDN_EUNSUPPORTED, "sample_pdf: n_samples + n_importance > %d", kMaxFine);
    if (a.z_fine && !a.z) return fail(IDN_EINVAL, "sample_pdf: the merged depths need the coarse depths z");
    hipLaunchKernelGGL(sample_pdf_kernel, dim3((unsigned)((a.n_rays + 3) / 4)), dim3(256), 0, s, a);
    IDN_HIP_CHECK(hipGetLastError());
    return IDN_OK;
}

}  // namespace idn
