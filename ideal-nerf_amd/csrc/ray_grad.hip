// Gradient of one render pass with respect to its ray records (pose refinement).  gfx950.
//
//   d_x[n_rays * S, pts_ch + views_ch]   dL / d [gamma_L(point) | gamma_Lv(view direction)] of every point (dx_kernel,
//      train.hip); L = multires (10: 63 columns), Lv = multires_views (4: 27 columns) of the network, [n_rays * S, 90] by default
//   d_rays[:, 6] on entry dL / d |rays_d| of raw2outputs' dists = dz * |rays_d| (composite_bwd_kernel<., true>, baseline.py:341-343)
//   -> d_rays[n_rays, 11] in the layout of the ray record: 0:3 d rays_o, 3:6 d rays_d, 6:8 zeros (near / far carry no
//      gradient), 8:11 d viewdirs
//
// Encoding backward (helper.py:174-224, audio_exp_nerf.py:331,380): per point p and axis a
//   d pts[a] = dx[a] + sum_k 2^k (cos(2^k p_a) dx_sin[k, a] - sin(2^k p_a) dx_cos[k, a]),  k < L   (k < Lv: view direction;
//   with no band the sum is empty and d pts = dx)
// with the point recomputed as the forward does (point_of<kModeRays>: product and sum rounded separately; this file is
// built with -ffp-contract=off; 2^k p is exact) and accurate sinf / cosf.  Then per ray
//   d rays_o = sum_s d pts_s,  d rays_d = sum_s z_s d pts_s + d_norm rays_d / |rays_d|,  d viewdirs = sum_s d dir_s.
// Depths carry no gradient (coarse depths depend on near / far alone, fine depths are detached upstream, :345).
//
// One wave per ray (one 64-thread workgroup), lane l owns samples l, l + 64, ... (up to 8 at S = 512).  The d_x rows of a
// chunk of 64 samples are 64 * 90 contiguous floats (64 * cols for a narrower network): the wave copies them to LDS with
// coalesced loads (row pitch 91 -- cols + 1, cols being even --, odd: lane-per-row reads are conflict-free), then each lane reads its row.  Reduction: a lane adds its samples in sample
// order, the lanes are added by a fixed xor tree, both in fp64 -- no atomics, the same order wherever the ray sits in the grid.
#include "idn_internal.h"

namespace idn {

constexpr int kRgMaxCols = IDN_PTS_CH + IDN_VIEWS_CH;   // 90: the widest rows
constexpr int kRgMaxPitch = kRgMaxCols + 1;             // 91
static_assert(64 * kRgMaxPitch * 4 <= 64 * 1024, "a chunk of rows fits the LDS of a workgroup");

__device__ __forceinline__ double rg_xor_dd(double v, int mask) {
    int lo = __double2loint(v), hi = __double2hiint(v);
    lo = __shfl_xor(lo, mask, 64);
    hi = __shfl_xor(hi, mask, 64);
    return __hiloint2double(hi, lo);
}

// L / Lv: the bands of the point / direction encoding (0..10, 0..4), uniform over the grid
__global__ __launch_bounds__(64) void ray_grad_kernel(const float* d_x, int L, int Lv, const float* rays, const float* z,
                                                      long n_rays, int S, float* d_rays) {
    __shared__ float rows[64 * kRgMaxPitch];
    const int pts_ch = 3 + 6 * L, kRgCols = pts_ch + 3 + 6 * Lv, kRgPitch = kRgCols + 1;   // (3 + 6 L) + (3 + 6 Lv) is even
    const int lane = threadIdx.x;
    const long ray = blockIdx.x;
    if (ray >= n_rays) return;
    const float* rr = rays + ray * IDN_RAY_FLOATS;
    const float o[3] = {rr[0], rr[1], rr[2]}, d[3] = {rr[3], rr[4], rr[5]}, v[3] = {rr[8], rr[9], rr[10]};
    // the view direction's encoding is the ray's: its 4 x 3 sines and cosines once per lane (those of bands the network does
    // not have are computed and not used)
    float vs[4][3], vc[4][3];
#pragma unroll
    for (int k = 0; k < 4; ++k)
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            const float t = v[a] * (float)(1 << k);
            vs[k][a] = sinf(t);
            vc[k][a] = cosf(t);
        }
    double go[3] = {0, 0, 0}, gd[3] = {0, 0, 0}, gv[3] = {0, 0, 0};
    const float* xr = d_x + ray * (long)S * kRgCols;
    for (int s0 = 0; s0 < S; s0 += 64) {
        const int cnt = S - s0 < 64 ? S - s0 : 64;
        const float* src = xr + (long)s0 * kRgCols;
        __syncthreads();   // the previous chunk has been read
        for (int e = lane; e < cnt * kRgCols; e += 64) {
            const int r = e / kRgCols;
            rows[r * kRgPitch + (e - r * kRgCols)] = src[e];
        }
        __syncthreads();
        if (lane < cnt) {
            const float* g = rows + lane * kRgPitch;
            const float zs = z[ray * S + s0 + lane];
#pragma unroll
            for (int a = 0; a < 3; ++a) {
                const float p = o[a] + d[a] * zs;
                float acc = g[a];
                for (int k = 0; k < L; ++k) {   // (uniform trip count; the same additions in the same order as ten unrolled bands)
                    const float f = (float)(1 << k), t = p * f;
                    acc += f * (cosf(t) * g[3 + 6 * k + a] - sinf(t) * g[6 + 6 * k + a]);
                }
                go[a] += (double)acc;
                gd[a] += (double)zs * (double)acc;
                const float* gq = g + pts_ch;
                float accv = gq[a];
#pragma unroll
                for (int k = 0; k < IDN_MAX_MULTIRES_VIEWS; ++k)
                    if (k < Lv) accv += (float)(1 << k) * (vc[k][a] * gq[3 + 6 * k + a] - vs[k][a] * gq[6 + 6 * k + a]);
                gv[a] += (double)accv;
            }
        }
    }
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1)
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            go[a] += rg_xor_dd(go[a], m);
            gd[a] += rg_xor_dd(gd[a], m);
            gv[a] += rg_xor_dd(gv[a], m);
        }
    if (lane == 0) {
        const float dn = sqrtf((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]);   // as composite_bwd_kernel
        float* out = d_rays + ray * IDN_RAY_FLOATS;
        const double gn = dn > 0.f ? (double)out[6] / (double)dn : 0.0;
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            out[a] = (float)go[a];
            out[3 + a] = (float)(gd[a] + gn * (double)d[a]);
            out[8 + a] = (float)gv[a];
        }
        out[6] = 0.f;
        out[7] = 0.f;
    }
}

int launch_ray_grad(const float* d_x, int pts_ch, int views_ch, const float* rays, const float* z, int64_t n_rays, int S,
                    float* d_rays, hipStream_t s) {
    if (n_rays <= 0) return IDN_OK;
    if (!widths_ok(pts_ch, views_ch)) return fail(IDN_EINVAL, "ray_grad: row widths %d / %d", pts_ch, views_ch);
    if (n_rays > 0x7fffffffLL) return fail(IDN_EUNSUPPORTED, "ray_grad: n_rays %lld exceeds 2^31-1 per launch", (long long)n_rays);
    hipLaunchKernelGGL(ray_grad_kernel, dim3((unsigned)n_rays), dim3(64), 0, s, d_x, (pts_ch - 3) / 6, (views_ch - 3) / 6, rays, z,
                       (long)n_rays, S, d_rays);
    IDN_HIP_CHECK(hipGetLastError());
    return IDN_OK;
}

}  // namespace idn
