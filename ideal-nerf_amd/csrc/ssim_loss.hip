// SSIM as a training loss on contiguous p x p patches of a ray batch (gfx950): the patch pixel indices, the loss and its gradient
// (include/idealnerf.h: idealnerf_patch_pixels, idealnerf_ssim_patch_fwd, idealnerf_ssim_patch_bwd).  The index is the scorer's
// (metrics.hip, frame_scores_tiles): the same eleven fp32 weights widened to fp64, C1 = 1e-4, C2 = 9e-4, "valid" windows, all five
// window moments and the index in fp64, and the same order of additions inside a window (along the row, then down the column).
//
//   patch_pixels:      one thread per pixel of the k patches; the origins travel as kernel arguments.
//   ssim_patch_fwd:    one workgroup per PATCH; it stages one channel of both images in LDS (2 x 48^2 fp32 = 18 KiB), every lane
//                      evaluates its windows' moments from LDS (121 taps each: no row-filtered planes, which at p = 48 would not
//                      fit beside the tiles) and adds the index; the three channels run one after the other in the same lanes.
//   ssim_patch_final:  out[k] = 1 - mean(out[0 .. k)), one lane, patches in index order.
//   ssim_patch_bwd:    one workgroup per (patch, channel): the window moments again, by the same function and so to the same bits,
//                      then per window the coefficients A = dS/d mu_x, B = dS/d E[xx], C = dS/d E[xt] into three fp64 LDS planes
//                      (3 x 38^2 x 8 = 33.8 KiB), then every PIXEL gathers from the at most 121 windows that cover it:
//                          d_pred = -((g / k) / (3 (p - 10)^2)) (sum w A + 2 x sum w B + t sum w C),  w = w_row w_col
//                      rounded once to fp32.  No atomics: a pixel's sum is one lane's, rows of windows in index order.
//
// No floating-point atomics anywhere: a lane adds its windows in index order, a wave folds its lanes by a fixed shuffle tree, the
// waves of a workgroup are added in index order.  A patch is one workgroup's (fwd) or three workgroups' (bwd) work and reads no
// other patch: its result does not depend on its neighbours in the call.  (g / k) is formed first, so that a call with g = k on k
// patches scales exactly as a call with g = 1 on one.)
#include "idn_internal.h"

namespace idn {

constexpr int kWinL = 11;
constexpr int kPatchMax = IDN_PATCH_MAX_P;              // 48
constexpr int kPatchWinMax = kPatchMax - kWinL + 1;     // 38
constexpr int kLossThreads = 256;
constexpr int kLossWaves = kLossThreads / 64;

// exp(-(k - 5)^2 / (2 * 1.5^2)), k = 0..10, normalised in fp64 and rounded to fp32: metrics.hip's table, repeated
__constant__ const float kGaussL[kWinL] = {0.00102838012f, 0.00759875821f, 0.0360007733f, 0.109360687f, 0.213005543f, 0.266011715f,
                                           0.213005543f,   0.109360687f,   0.0360007733f, 0.00759875821f, 0.00102838012f};

__global__ __launch_bounds__(256) void patch_pixels_kernel(idn_patch_set set, int W, long long* __restrict__ sel) {
    const int pp = set.p * set.p;
    const int idx = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (idx >= set.n_patches * pp) return;
    const int k = idx / pp, rem = idx - k * pp;
    const int r = rem / set.p, c = rem - r * set.p;
    sel[idx] = (long long)(set.oy[k] + r) * (long long)W + (long long)(set.ox[k] + c);
}

// The five moments of the window whose top-left corner is (r, c) of the staged channel: along each row first (hm of
// frame_scores_tiles), then down the column, in the scorer's order of additions.
__device__ inline void window_moments(const float (*sx)[kPatchMax], const float (*st)[kPatchMax], int r, int c, double mo[5]) {
#pragma unroll
    for (int q = 0; q < 5; ++q) mo[q] = 0.0;
    for (int i = 0; i < kWinL; ++i) {
        double a = 0.0, b = 0.0, aa = 0.0, bb = 0.0, ab = 0.0;
#pragma unroll
        for (int k = 0; k < kWinL; ++k) {
            const double w = (double)kGaussL[k], xv = (double)sx[r + i][c + k], tv = (double)st[r + i][c + k];
            a += w * xv;
            b += w * tv;
            aa += w * (xv * xv);
            bb += w * (tv * tv);
            ab += w * (xv * tv);
        }
        const double w = (double)kGaussL[i];
        mo[0] += w * a; mo[1] += w * b; mo[2] += w * aa; mo[3] += w * bb; mo[4] += w * ab;
    }
}

__device__ inline void stage_channel(const float* __restrict__ pred, const float* __restrict__ truth, size_t base, int p, int ch,
                                     float (*sx)[kPatchMax], float (*st)[kPatchMax], int tid) {
    for (int idx = tid; idx < p * p; idx += kLossThreads) {
        const int r = idx / p, c = idx - r * p;
        sx[r][c] = pred[(base + (size_t)idx) * 3 + ch];
        st[r][c] = truth[(base + (size_t)idx) * 3 + ch];
    }
}

__global__ __launch_bounds__(kLossThreads) void ssim_patch_fwd_kernel(const float* __restrict__ pred, const float* __restrict__ truth, int p,
                                                                     double* __restrict__ out) {
    __shared__ float sx[kPatchMax][kPatchMax];
    __shared__ float st[kPatchMax][kPatchMax];
    __shared__ double red[kLossWaves];
    const int tid = threadIdx.x;
    const int nw = p - kWinL + 1;
    const size_t base = (size_t)blockIdx.x * (size_t)(p * p);
    double acc = 0.0;
    for (int ch = 0; ch < 3; ++ch) {
        if (ch) __syncthreads();   // the previous channel's windows have been read
        stage_channel(pred, truth, base, p, ch, sx, st, tid);
        __syncthreads();
        for (int idx = tid; idx < nw * nw; idx += kLossThreads) {
            const int r = idx / nw, c = idx - r * nw;
            double mo[5];
            window_moments(sx, st, r, c, mo);
            const double C1 = 1e-4, C2 = 9e-4;
            const double mx = mo[0], mt = mo[1];
            const double vx = mo[2] - mx * mx, vt = mo[3] - mt * mt, cov = mo[4] - mx * mt;
            acc += ((2.0 * mx * mt + C1) * (2.0 * cov + C2)) / ((mx * mx + mt * mt + C1) * (vx + vt + C2));
        }
    }
    // ---- lanes -> wave (shuffle tree) -> workgroup (waves in order)
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) acc += __shfl_down(acc, d, 64);
    if ((tid & 63) == 0) red[tid >> 6] = acc;
    __syncthreads();
    if (tid == 0) {
        double v = red[0];
#pragma unroll
        for (int w = 1; w < kLossWaves; ++w) v += red[w];
        out[blockIdx.x] = v / (3.0 * (double)(nw * nw));
    }
}

__global__ __launch_bounds__(64) void ssim_patch_final_kernel(int n_patches, double* __restrict__ out) {
    if (threadIdx.x != 0) return;
    double v = 0.0;
    for (int k = 0; k < n_patches; ++k) v += out[k];
    out[n_patches] = 1.0 - v / (double)n_patches;
}

__global__ __launch_bounds__(kLossThreads) void ssim_patch_bwd_kernel(const float* __restrict__ pred, const float* __restrict__ truth, int p,
                                                                     double scale, float* __restrict__ d_pred) {
    __shared__ float sx[kPatchMax][kPatchMax];
    __shared__ float st[kPatchMax][kPatchMax];
    __shared__ double co[3][kPatchWinMax][kPatchWinMax];   // A, B, C of every window
    static_assert(2 * sizeof(float) * kPatchMax * kPatchMax + 3 * sizeof(double) * kPatchWinMax * kPatchWinMax <= 65536,
                  "static LDS of one workgroup");
    const int tid = threadIdx.x;
    const int nw = p - kWinL + 1;
    const int patch = (int)blockIdx.x / 3, ch = (int)blockIdx.x - patch * 3;
    const size_t base = (size_t)patch * (size_t)(p * p);
    stage_channel(pred, truth, base, p, ch, sx, st, tid);
    __syncthreads();
    for (int idx = tid; idx < nw * nw; idx += kLossThreads) {
        const int r = idx / nw, c = idx - r * nw;
        double mo[5];
        window_moments(sx, st, r, c, mo);
        const double C1 = 1e-4, C2 = 9e-4;
        const double mx = mo[0], mt = mo[1];
        const double vx = mo[2] - mx * mx, vt = mo[3] - mt * mt, cov = mo[4] - mx * mt;
        const double a1 = 2.0 * mx * mt + C1, a2 = 2.0 * cov + C2, b1 = mx * mx + mt * mt + C1, b2 = vx + vt + C2;
        const double S = (a1 * a2) / (b1 * b2);
        // S(mu_x, E[xx], E[xt]) with mu_t, E[tt] fixed: vx = E[xx] - mu_x^2, cov = E[xt] - mu_x mu_t
        co[0][r][c] = (2.0 * mt * (a2 - a1)) / (b1 * b2) - (2.0 * mx * S) / b1 + (2.0 * mx * S) / b2;
        co[1][r][c] = -S / b2;
        co[2][r][c] = (2.0 * a1) / (b1 * b2);
    }
    __syncthreads();
    for (int idx = tid; idx < p * p; idx += kLossThreads) {
        const int y = idx / p, x = idx - y * p;
        // the windows (r, c) that cover pixel (y, x): r in [y - 10, y] and [0, nw), the pixel being tap (y - r, x - c) of them
        const int r_lo = y - (kWinL - 1) > 0 ? y - (kWinL - 1) : 0, r_hi = y < nw - 1 ? y : nw - 1;
        const int c_lo = x - (kWinL - 1) > 0 ? x - (kWinL - 1) : 0, c_hi = x < nw - 1 ? x : nw - 1;
        double sa = 0.0, sb = 0.0, sc = 0.0;
        for (int r = r_lo; r <= r_hi; ++r) {
            double ra = 0.0, rb = 0.0, rc = 0.0;
            for (int c = c_lo; c <= c_hi; ++c) {
                const double w = (double)kGaussL[x - c];
                ra += w * co[0][r][c];
                rb += w * co[1][r][c];
                rc += w * co[2][r][c];
            }
            const double w = (double)kGaussL[y - r];
            sa += w * ra; sb += w * rb; sc += w * rc;
        }
        const double xv = (double)sx[y][x], tv = (double)st[y][x];
        d_pred[(base + (size_t)idx) * 3 + ch] = (float)(-scale * (sa + 2.0 * xv * sb + tv * sc));
    }
}

int launch_patch_pixels(const idn_patch_set& set, int W, long long* sel, hipStream_t s) {
    const int n = set.n_patches * set.p * set.p;
    hipLaunchKernelGGL(patch_pixels_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, set, W, sel);
    IDN_HIP_CHECK(hipGetLastError());
    return IDN_OK;
}

int launch_ssim_patch_fwd(const float* pred, const float* truth, int n_patches, int p, double* out, hipStream_t s) {
    hipLaunchKernelGGL(ssim_patch_fwd_kernel, dim3((unsigned)n_patches), dim3(kLossThreads), 0, s, pred, truth, p, out);
    IDN_HIP_CHECK(hipGetLastError());
    hipLaunchKernelGGL(ssim_patch_final_kernel, dim3(1), dim3(64), 0, s, n_patches, out);
    IDN_HIP_CHECK(hipGetLastError());
    return IDN_OK;
}

int launch_ssim_patch_bwd(const float* pred, const float* truth, int n_patches, int p, float g, float* d_pred, hipStream_t s) {
    const int nw = p - kWinL + 1;
    const double scale = ((double)g / (double)n_patches) / (3.0 * (double)(nw * nw));
    hipLaunchKernelGGL(ssim_patch_bwd_kernel, dim3((unsigned)(n_patches * 3)), dim3(kLossThreads), 0, s, pred, truth, p, scale, d_pred);
    IDN_HIP_CHECK(hipGetLastError());
    return IDN_OK;
}

}  // namespace idn
