// Backward of one render pass (coarse or fine) for the training step
// (NeRFs/HeadNeRF/train/audio_exp_nerf.py:534-552: loss.backward() through raw2outputs,
// FaceNeRF and the per-frame conditioning).  gfx950, fp32 MFMA.
//
//   composite_bwd     d(rgb_map, rgb_fg, last_weight, acc) -> d raw           (one wave per ray)
//   delta chain       all delta_l = (delta_{l+1} . W_{l+1}) (.) [a_l > 0] in one fused kernel (mlp_f32_bwd.hip)
//   dW products       dW_l = delta_l^T . a_{l-1} and db_l = sum_p delta_l: dw_gemm.hip, scheduled by DwPass (dw_gemm.h)
//   fold_bwd          conditioning columns of W0 / W5 / Wv0 and d aud, d latent
//   ray gradient      (idealnerf_pass_bwd_rays) after all of that: dx_kernel into the workspace, then ray_grad.hip; the compositing
//                     backward's kNorm variant supplies dL / d |rays_d|
//   frozen network    (no gradient tensors: idealnerf_pass_bwd_cond) instead of the dW products, colsum_rows / colsum_finish on
//                     dA[0] and dA[5], and the d cond range of fold_bwd alone; with d expr or views_linears.0's bias gradient
//                     wanted (idealnerf_pass_bwd_ex) also on the 128 delta columns of dV0, over the pass's real rows
//
// Activations come from the training variant of the MLP kernel as row-major matrices
// (idn_internal.h, "activation slab").  Everything is deterministic: no float atomics.
#include "dw_gemm.h"
#include "march.h"
#include <cstdlib>

namespace idn {

// ---------------------------------------------------------------------------
// compositing backward (baseline.py:325-375 differentiated; cumprod's gradient as
// PyTorch computes it when no factor is zero: reverse cumsum(grad * out) / input).
// ---------------------------------------------------------------------------
__device__ __forceinline__ double shfl_up_dd(double v, int delta) {
    int lo = __double2loint(v), hi = __double2hiint(v);
    lo = __shfl_up(lo, delta, 64);
    hi = __shfl_up(hi, delta, 64);
    return __hiloint2double(hi, lo);
}
__device__ __forceinline__ double shfl_down_dd(double v, int delta) {
    int lo = __double2loint(v), hi = __double2hiint(v);
    lo = __shfl_down(lo, delta, 64);
    hi = __shfl_down(hi, delta, 64);
    return __hiloint2double(hi, lo);
}
__device__ __forceinline__ double shfl_xor_dd(double v, int mask) {
    int lo = __double2loint(v), hi = __double2hiint(v);
    lo = __shfl_xor(lo, mask, 64);
    hi = __shfl_xor(hi, mask, 64);
    return __hiloint2double(hi, lo);
}

// kNorm: also the per-ray gradient of dists = dz * |rays_d| with respect to the norm (baseline.py:341-343; the ray's last
// sample is left out: across its 1e10 spacing alpha is saturated).  The other outputs are the same instructions either way.
template <int SPL, bool kNorm = false>
__global__ __launch_bounds__(256) void composite_bwd_kernel(CompBwdArgs a) {
    const int lane = threadIdx.x & 63;
    const long ray = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (ray >= a.n_rays) return;
    const int S = a.S;
    const float* rr = a.rays + ray * IDN_RAY_FLOATS;
    const float dn = sqrtf((rr[3] * rr[3] + rr[4] * rr[4]) + rr[5] * rr[5]);
    const float4* rawr = a.raw + ray * S;
    const float* zr = a.z + ray * S;
    float gr = 0, gg = 0, gb = 0, fr = 0, fg = 0, fb = 0, glw = 0, gacc = 0;
    if (a.g_rgb) { gr = a.g_rgb[ray * 3]; gg = a.g_rgb[ray * 3 + 1]; gb = a.g_rgb[ray * 3 + 2]; }
    if (a.g_fg) { fr = a.g_fg[ray * 3]; fg = a.g_fg[ray * 3 + 1]; fb = a.g_fg[ray * 3 + 2]; }
    if (a.g_lw) glw = a.g_lw[ray];
    if (a.g_acc) gacc = a.g_acc[ray];

    float zs[SPL + 1];
    float4 rw[SPL];
#pragma unroll
    for (int i = 0; i < SPL; ++i) {
        const int s = lane * SPL + i;
        zs[i] = s < S ? zr[s] : 0.f;
        rw[i] = s < S ? rawr[s] : make_float4(0.f, 0.f, 0.f, 0.f);
    }
    zs[SPL] = __shfl_down(zs[0], 1, 64);
    float alpha[SPL], tf[SPL], ex[SPL], dist[SPL];
    double local = 1.0;
#pragma unroll
    for (int i = 0; i < SPL; ++i) {
        const int s = lane * SPL + i;
        float d = (s >= S - 1) ? 1e10f : (zs[i + 1] - zs[i]);
        d = d * dn;
        const float e = expf(-(fmaxf(rw[i].w, 0.0f) + 1e-6f) * d);
        dist[i] = d;
        ex[i] = e;
        alpha[i] = (s < S) ? 1.0f - e : 0.0f;
        tf[i] = (s < S) ? (1.0f - (1.0f - e)) + 1e-10f : 1.0f;
        local *= (double)tf[i];
    }
    // exclusive prefix product over lanes
    double incl = local;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const double o = shfl_up_dd(incl, d);
        if (lane >= d) incl *= o;
    }
    double run = shfl_up_dd(incl, 1);
    if (lane == 0) run = 1.0;
    float T[SPL], w[SPL], dw[SPL], cr[SPL], cg[SPL], cb[SPL];
    double lsum = 0.0;  // sum of dw*w over this lane's samples
#pragma unroll
    for (int i = 0; i < SPL; ++i) {
        const int s = lane * SPL + i;
        T[i] = (float)run;
        w[i] = alpha[i] * T[i];
        run *= (double)tf[i];
        dw[i] = 0.f;
        cr[i] = cg[i] = cb[i] = 0.f;
        if (s < S) {
            if (s == S - 1) {
                cr[i] = a.bc[ray * 3]; cg[i] = a.bc[ray * 3 + 1]; cb[i] = a.bc[ray * 3 + 2];
                dw[i] = (gr * cr[i] + gg * cg[i] + gb * cb[i]) + glw + gacc;
            } else {
                cr[i] = 1.0f / (1.0f + expf(-rw[i].x));
                cg[i] = 1.0f / (1.0f + expf(-rw[i].y));
                cb[i] = 1.0f / (1.0f + expf(-rw[i].z));
                dw[i] = ((gr + fr) * cr[i] + (gg + fg) * cg[i] + (gb + fb) * cb[i]) + gacc;
            }
            lsum += (double)dw[i] * (double)w[i];
        }
    }
    // suffix sums of dw*w, added up from the ray's far end: sum_{t > s} dw_t w_t then keeps its own relative precision however small
    // it is beside the ray's total (as total - inclusive prefix it carried 1e-16 of the total, and a sample behind an opaque one
    // got a d sigma of that size times dist instead of one that vanishes with its transmittance)
    double lsfx = lsum;   // inclusive suffix over the lanes
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const double o = shfl_down_dd(lsfx, d);
        if (lane + d < 64) lsfx += o;
    }
    double after = shfl_down_dd(lsfx, 1);  // sum over later lanes
    if (lane == 63) after = 0.0;
    double sfx[SPL];                       // sum_{t > s} dw_t w_t
#pragma unroll
    for (int i = SPL - 1; i >= 0; --i) {
        sfx[i] = after;
        after += (double)dw[i] * (double)w[i];   // (zero beyond the ray's end)
    }
    double nsum = 0.0;           // kNorm: this lane's share of dL / d |rays_d|
#pragma unroll
    for (int i = 0; i < SPL; ++i) {
        const int s = lane * SPL + i;
        if (s < S) {
            const float dalpha = dw[i] * T[i] - (float)(sfx[i] / (double)tf[i]);
            const float dsig = (rw[i].w > 0.f) ? dalpha * ex[i] * dist[i] : 0.f;
            if constexpr (kNorm) {
                if (s < S - 1)
                    nsum += (double)dalpha * (double)ex[i] * (double)(fmaxf(rw[i].w, 0.0f) + 1e-6f) * (double)(zs[i + 1] - zs[i]);
            }
            const long p = ray * S + s;
            a.d_sig[p * a.ld_sig] = dsig;
            float d0 = 0.f, d1 = 0.f, d2 = 0.f;
            if (s < S - 1) {
                d0 = w[i] * (gr + fr) * cr[i] * (1.0f - cr[i]);
                d1 = w[i] * (gg + fg) * cg[i] * (1.0f - cg[i]);
                d2 = w[i] * (gb + fb) * cb[i] * (1.0f - cb[i]);
            }
            a.d_rgb[p * a.ld_rgb + 0] = d0;
            a.d_rgb[p * a.ld_rgb + 1] = d1;
            a.d_rgb[p * a.ld_rgb + 2] = d2;
        }
    }
    if constexpr (kNorm) {
#pragma unroll
        for (int m = 32; m >= 1; m >>= 1) nsum += shfl_xor_dd(nsum, m);
        if (lane == 0) a.d_norm[ray * a.ld_norm] = (float)nsum;
    }
}

// ---------------------------------------------------------------------------
// conditioning fold backward
//   dW0[:, 63+c] = db0'[n] cond[c];  dW5[:, 63+c] = db5'[n] cond[c];  dWv0[:, 283+e] = dbv'[n] expr3[e]
//   d cond[c] = sum_n W0[n][63+c] db0'[n] + W5[n][63+c] db5'[n]   -> d aud, d latent (accumulated)
//   d expr[e] = (d cond[dim_aud+e] + sum_n Wv0[n][283+e] dbv'[n]) / 3   (expr * 1 / 3 enters all three layers, face_nerf.py:49)
// (63 and 283 at the default widths: the network's pts_ch and 256 + views_ch, idn_internal.h)
// ---------------------------------------------------------------------------
// (FoldBwdArgs: idn_internal.h)
__device__ __forceinline__ float cond_val(const FoldBwdArgs& d, int c) {
    if (c < d.p.dim_aud) return d.aud[c];
    c -= d.p.dim_aud;
    if (c < d.p.dim_expr) return d.expr[c] * 1.0f / 3.0f;
    c -= d.p.dim_expr;
    return d.latent[c];
}
// kCondOnly: the launch covers the d cond index range alone (a frozen network: bwd_tail without gradient tensors) -- gW0 / gW5 /
// gWv0 are never touched, dbv only with d_expr
template <bool kCondOnly>
__global__ void fold_bwd_kernel(FoldBwdArgs d) {
    const int C = d.p.dim_aud + d.p.dim_expr + d.p.dim_latent;
    const int PC = pts_ch_of(d.p), VC = views_ch_of(d.p);
    const int ld0 = PC + C, ld5 = PC + C + IDN_W, ldv = IDN_W + VC + d.p.dim_expr;
    const int idx = blockIdx.x * blockDim.x + threadIdx.x + (kCondOnly ? IDN_W * C + (IDN_W / 2) * d.p.dim_expr : 0);
    const int n_outer = IDN_W * C;
    if (!kCondOnly && idx < n_outer) {
        const int n = idx / C, c = idx % C;
        const float cv = cond_val(d, c);
        d.gW0[(long)n * ld0 + PC + c] = d.db0[n] * cv;
        d.gW5[(long)n * ld5 + PC + c] = d.db5[n] * cv;
    } else if (!kCondOnly && idx < n_outer + (IDN_W / 2) * d.p.dim_expr) {
        const int k = idx - n_outer, n = k / d.p.dim_expr, e = k % d.p.dim_expr;
        d.gWv0[(long)n * ldv + IDN_W + VC + e] = d.dbv[n] * (d.expr[e] * 1.0f / 3.0f);
    } else {
        // d cond[c]: one wavefront per conditioning column, the lanes split the 256 rows (a thread per column
        // walked them as one chain of dependent strided loads: 65 us)
        const int rel = idx - n_outer - (IDN_W / 2) * d.p.dim_expr;   // n_outer and 128 dim_expr are multiples of 64
        const int c = rel >> 6, lane = rel & 63;
        if (c >= C) return;
        double s = 0.0;
        for (int n = lane; n < IDN_W; n += 64)
            s += (double)d.p.pts_w[0][(long)n * ld0 + PC + c] * (double)d.db0[n] +
                 (double)d.p.pts_w[5][(long)n * ld5 + PC + c] * (double)d.db5[n];
#pragma unroll
        for (int m = 32; m >= 1; m >>= 1) s += shfl_xor_dd(s, m);
        // an expr column also feeds views_linears.0 (wave-uniform branch; never taken when d_expr is NULL)
        const int e = c - d.p.dim_aud;
        const bool want_expr = d.d_expr != nullptr && e >= 0 && e < d.p.dim_expr;
        double sv = 0.0;
        if (want_expr) {
            for (int n = lane; n < IDN_W / 2; n += 64)
                sv += (double)d.p.views_w[0][(long)n * ldv + IDN_W + VC + e] * (double)d.dbv[n];
#pragma unroll
            for (int m = 32; m >= 1; m >>= 1) sv += shfl_xor_dd(sv, m);
        }
        if (lane != 0) return;
        if (c < d.p.dim_aud) {
            if (d.d_aud) d.d_aud[c] += (float)s;
        } else if (c >= d.p.dim_aud + d.p.dim_expr) {
            if (d.d_latent) d.d_latent[c - d.p.dim_aud - d.p.dim_expr] += (float)s;
        } else if (want_expr) {
            d.d_expr[e] += (float)((s + sv) / 3.0);
        }
    }
}

// ---------------------------------------------------------------------------
// Column sums of two [rows, 256] fp32 matrices (row pitch 256): the bias gradients db0' / db5' the conditioning fold reads, for
// a pass whose weight gradients nobody wants.  Deterministic, no float atomics: workgroup (b, m) sums rows
// [b rows_per_block, (b + 1) rows_per_block) of matrix m in row order, one thread per column (a row is one coalesced 1 KB
// line), in fp64; colsum_finish_kernel adds the partial sums in block order.  Launched with 128 threads and one matrix
// (grid.y = 1) the pair sums columns 0..127 alone: views_linears.0's deltas in dV0, dbv'.
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(256) void colsum_rows_kernel(const float* m0, const float* m1, long rows, long rows_per_block, double* part) {
    const float* m = blockIdx.y ? m1 : m0;
    const long r0 = (long)blockIdx.x * rows_per_block;
    const long r1 = r0 + rows_per_block < rows ? r0 + rows_per_block : rows;
    const float* col = m + threadIdx.x;
    double acc = 0.0;
    long r = r0;
    for (; r + 8 <= r1; r += 8) {
        float v[8];
#pragma unroll
        for (int i = 0; i < 8; ++i) v[i] = col[(r + i) * 256];
#pragma unroll
        for (int i = 0; i < 8; ++i) acc += (double)v[i];
    }
    for (; r < r1; ++r) acc += (double)col[r * 256];
    part[((long)blockIdx.x * 2 + blockIdx.y) * 256 + threadIdx.x] = acc;
}
__global__ __launch_bounds__(256) void colsum_finish_kernel(const double* part, int blocks, float* out) {
    double acc = 0.0;   // out [2][256]: workgroup m finishes matrix m
    for (int b = 0; b < blocks; ++b) acc += part[((long)b * 2 + blockIdx.x) * 256 + threadIdx.x];
    out[blockIdx.x * 256 + threadIdx.x] = (float)acc;
}
constexpr int kCondColsumBlocks = 512;   // row blocks at the most: their fp64 partial sums and the 512 results fit the cpart pool
static_assert(512 + (size_t)kCondColsumBlocks * 512 * 2 <= kCpartPoolFloats, "the conditioning-only column sums fit the cpart pool");
size_t cond_colsums_workspace_bytes() { return (size_t)kCondColsumBlocks * 512 * sizeof(double); }

// The two column-sum steps of a frozen pass (bwd_tail without gradient tensors), and all of idealnerf_cond_colsums:
//   db [2][256] = the column sums of dA0 | dA5 over all Pp rows (dA0 null: the step is left out);
//   dbv [128]   = the column sums of dV0[:, 0:128] over the first P rows (dV0 null: left out).
// part: kCondColsumBlocks x 512 doubles, free again between the two steps (the stream orders them).
int launch_cond_colsums(const float* dA0, const float* dA5, const float* dV0, int64_t P, int64_t Pp, float* db, float* dbv,
                        double* part, hipStream_t s) {
    const int64_t chunks = Pp / 128;
    const int64_t rows_per_block = (chunks + kCondColsumBlocks - 1) / kCondColsumBlocks * 128;
    if (dA0) {
        const int blocks = (int)((Pp + rows_per_block - 1) / rows_per_block);
        hipLaunchKernelGGL(colsum_rows_kernel, dim3(blocks, 2), dim3(256), 0, s, dA0, dA5, (long)Pp, (long)rows_per_block, part);
        IDN_HIP_CHECK(hipGetLastError());
        hipLaunchKernelGGL(colsum_finish_kernel, dim3(2), dim3(256), 0, s, (const double*)part, blocks, db);
        IDN_HIP_CHECK(hipGetLastError());
    }
    // dbv' [128]: the same two kernels, 128 threads wide, on dV0's delta columns and the real rows alone
    if (dV0) {
        const int blocks = (int)((P + rows_per_block - 1) / rows_per_block);
        hipLaunchKernelGGL(colsum_rows_kernel, dim3(blocks, 1), dim3(128), 0, s, dV0, dV0, (long)P, (long)rows_per_block, part);
        IDN_HIP_CHECK(hipGetLastError());
        hipLaunchKernelGGL(colsum_finish_kernel, dim3(1), dim3(128), 0, s, (const double*)part, blocks, dbv);
        IDN_HIP_CHECK(hipGetLastError());
    }
    return IDN_OK;
}

// The conditioning fold's backward, both launches of bwd_tail and all of idealnerf_fold_bwd.  cond_only: the d cond range
// alone (fold_bwd_kernel<true>: a wavefront per conditioning column); else the whole index range, the outer products into
// the gradient tensors first.  A network without conditioning launches nothing.
int launch_fold_bwd(const FoldBwdArgs& f, bool cond_only, hipStream_t s) {
    const int C = f.p.dim_aud + f.p.dim_expr + f.p.dim_latent;
    if (cond_only) {
        if (C == 0) return IDN_OK;
        hipLaunchKernelGGL(fold_bwd_kernel<true>, dim3((C * 64 + 255) / 256), dim3(256), 0, s, f);
    } else {
        const int total = IDN_W * C + (IDN_W / 2) * f.p.dim_expr + C * 64;   // one wavefront per conditioning column at the end
        if (total == 0) return IDN_OK;
        hipLaunchKernelGGL(fold_bwd_kernel<false>, dim3((total + 255) / 256), dim3(256), 0, s, f);
    }
    IDN_HIP_CHECK(hipGetLastError());
    return IDN_OK;
}

// ---------------------------------------------------------------------------
// host orchestration
// ---------------------------------------------------------------------------
struct BwdWs {
    float *dA[8], *dV[2], *dV0, *dRGB, *part, *cpart, *wbwd;
    size_t bytes;
};
static BwdWs carve_bwd(char* base, int64_t p_pad) {
    BwdWs w;
    size_t off = 0;
    auto take = [&](size_t floats) {
        float* p = reinterpret_cast<float*>(base + off);
        off += al256(floats * 4);
        return p;
    };
    for (int l = 0; l < 8; ++l) w.dA[l] = take((size_t)p_pad * 256);  // delta of pts_linears.l (pre-activation)
    // delta of views_linears.2 | delta of views_linears.1 side by side in ONE 256-column matrix: their two 128 x 128 weight
    // gradients are then the diagonal blocks of a single 256 x 256 product (bwd_tail)
    w.dV[0] = take((size_t)p_pad * 256);
    w.dV[1] = w.dV[0] + 128;
    w.dV0 = take((size_t)p_pad * 256);
    w.dRGB = take((size_t)p_pad * 64);
    w.part = take(kPartPoolFloats);     // one slab per product of the pass: they are all reduced at its end (dw_gemm.h)
    w.cpart = take(kCpartPoolFloats);
    w.wbwd = take(bwd_stream_floats_x6());   // transposed weight stream of the delta chain (either pipe's: mlp_f32_bwd.hip)
    w.bytes = off;
    return w;
}

size_t bwd_workspace_bytes(int64_t n_points) {
    const int64_t p_pad = (n_points + 127) / 128 * 128;
    return carve_bwd(nullptr, p_pad).bytes;
}

// The backward's pipe for the delta chain and the 256 x 256 dW products: the six-piece bf16 arithmetic unless the process was
// started with IDN_BACKWARD_PIPE=f32 (read once; the A/B arm and the fallback, exercised by the GPU tests).
static int backward_pipe() {
    static const int v = [] {
        const char* e = getenv("IDN_BACKWARD_PIPE");
        return (e && e[0] == 'f' && e[1] == '3' && e[2] == '2' && e[3] == 0) ? kPipeF32 : kPipeX6;
    }();
    return v;
}

// The part of a backward that follows the head deltas (dRGB columns 0..2, dV0 column kSigmaChannel, zeros in the padding
// rows): the transposed weight stream, the delta chain, the weight / bias gradient products and the conditioning fold.
// launch_pass_bwd seeds the head deltas with the compositing backward, launch_facenerf_bwd with the caller's d raw.
// grads == nullptr (a frozen network): after the delta chain only what d aud / d latent need -- the column sums of dA[0] and
// dA[5] and the d cond range of the fold; no weight-gradient product runs and no gradient tensor is written.  There d_expr
// and d_vb [128] (views_linears.0's bias gradient, overwritten) need dbv': the column sums of dV0[:, 0:128] over the P real
// rows (the padding rows' deltas are whatever the chain made of rows the head deltas leave at zero: they stay out).
static int bwd_tail(const idn_facenerf_params& p, const idn_facenerf_grads* grads, const BwdCond& cond, const float* acts, int64_t P,
                    int64_t Pp, const BwdWs& w, hipStream_t s) {
    const int C = p.dim_aud + p.dim_expr + p.dim_latent;
    // the network's encoding widths: the leading dimensions of its three mixed-input tensors and the columns the narrow
    // takes keep of the 64-column products (the slab's x0 / dir matrices are 64 wide whatever the width)
    const int PC = pts_ch_of(p), VC = views_ch_of(p);
    const int ld0 = PC + C, ld5 = PC + C + IDN_W, ldv = IDN_W + VC + p.dim_expr;
    auto act = [&](int i) { return acts + (size_t)act_off(i) * Pp; };
    auto a_l = [&](int l) { return act(kActA1 + l - 1); };  // post-ReLU output of pts_linears.(l-1), l = 1..8
    auto v_l = [&](int l) { return act(kActV1 + l - 1); };  // post-ReLU output of views_linears.(l-1), l = 1..3
#define TRY(x) do { if (int e_ = (x)) return e_; } while (0)
    // All pre-activation deltas in one fused pass over the points (mlp_f32_bwd.hip): dV[0] = delta of
    // views_linears.2, dV[1] = views_linears.1, dV0[:, :128] = views_linears.0 (col 128 = d sigma), dA[l] = pts_linears.l
    const int pipe = backward_pipe();
    if (pipe == kPipeX6) {
        TRY(launch_pack_bf16x6_bwd(p, w.wbwd, s));
        TRY(launch_delta_chain_x6(w.wbwd, acts, Pp, w.dRGB, w.dV0, w.dV[0], w.dV[1], w.dA, s));
    } else {   // (the workspace's stream buffer is sized for the larger of the two streams)
        TRY(launch_pack_f32_bwd(p, w.wbwd, s));
        TRY(launch_delta_chain(w.wbwd, acts, Pp, w.dRGB, w.dV0, w.dV[0], w.dV[1], w.dA, s));
    }
    if (!grads) {
        const bool want_dbv = cond.d_expr != nullptr || cond.d_vb != nullptr;
        if (C == 0 && !want_dbv) return IDN_OK;
        float* db = w.cpart;                                        // [2][256]: db0', db5'
        double* part = reinterpret_cast<double*>(w.cpart + 512);    // [blocks][2][256] (the pool is 256-byte aligned)
        // dbv' [128] over the real rows alone; the result goes to the caller's buffer or, with none, to the partial-product
        // pool this plan never uses
        float* dbv = cond.d_vb ? cond.d_vb : w.part;
        TRY(launch_cond_colsums(C > 0 ? w.dA[0] : nullptr, w.dA[5], want_dbv ? w.dV0 : nullptr, P, Pp, db, dbv, part, s));
        const FoldBwdArgs f{p, cond.aud, cond.expr, cond.latent, db, db + 256, dbv, nullptr, nullptr, nullptr, cond.d_aud, cond.d_latent, cond.d_expr};
        return launch_fold_bwd(f, true, s);
    }
    const idn_facenerf_grads& gr = *grads;
    // weight and bias gradients: dW_l = delta_l^T a_{l-1} (contraction over the points), db_l = column sums.  The products in
    // kPassProducts' order (dw_gemm.h), each followed by the blocks of it that become gradients.
    DwPass q(w.part, kPartPoolFloats, w.cpart, kCpartPoolFloats, Pp, pipe, kX6ItemsPerPass, s);
    DwProduct h;
    TRY(q.product(w.dRGB, 64, 64, v_l(3), 128, 128, true, &h));
    TRY(q.take_colsum(h, 0, 3, gr.rgb_b));
    TRY(q.take(h, 0, 0, 3, 128, gr.rgb_w, 128));
    // views_linears.2 and .1 (128 x 128 each): on the bf16 pipe ONE 256 x 256 launch whose A is the side-by-side delta matrix and
    // whose B columns come from the two activation matrices (v2 | v1) -- the weight gradients are its diagonal blocks, and 1 KB per
    // point and layer is read once by a kernel that runs at the HBM rate (two fp32-MFMA launches took 1.7x as long).  The
    // off-diagonal blocks are computed and dropped.
    if (pipe == kPipeX6) {
        TRY(q.product(w.dV[0], 256, 256, v_l(2), 128, 256, true, &h, v_l(1)));
        TRY(q.take_colsum(h, 0, 128, gr.views_b[2]));
        TRY(q.take_colsum(h, 128, 128, gr.views_b[1]));
        TRY(q.take(h, 0, 0, 128, 128, gr.views_w[2], 128));
        TRY(q.take(h, 128, 128, 128, 128, gr.views_w[1], 128));
    } else {
        for (int l = 2; l >= 1; --l) {
            TRY(q.product(w.dV[2 - l], 256, 128, v_l(l), 128, 128, true, &h));
            TRY(q.take_colsum(h, 0, 128, gr.views_b[l]));
            TRY(q.take(h, 0, 0, 128, 128, gr.views_w[l], 128));
        }
    }
    // views_linears.0 and alpha_linear against a8 in ONE 256 x 256 product: A = the 256-column matrix dV0, whose columns 0..127
    // are views_linears.0's deltas and whose column 128 is d sigma (alpha_linear's delta); columns 129..255 are never written --
    // whatever they hold only reaches output rows 129..255, which are not read.  (It replaces a 128 x 256 fp32-MFMA product and
    // a weighted column sum that read dV0 and a8 once each.)  The direction-encoding columns stay a product of their own.
    TRY(q.product(w.dV0, 256, 256, a_l(8), 256, 256, true, &h));
    TRY(q.take_colsum(h, 0, 128, gr.views_b[0]));
    TRY(q.take_colsum(h, kSigmaChannel, 1, gr.alpha_b));
    TRY(q.take(h, 0, 0, 128, 256, gr.views_w[0], ldv));
    TRY(q.take(h, kSigmaChannel, 0, 1, 256, gr.alpha_w, 256));
    TRY(q.product(w.dV0, 256, 128, act(kActDir), 64, 64, false, &h));
    TRY(q.take(h, 0, 0, 128, VC, gr.views_w[0] + IDN_W, ldv));
    for (int l = 7; l >= 1; --l) {   // pts_linears.l; the skip layer's input is [encoding | conditioning | a5]: two products
        TRY(q.product(w.dA[l], 256, 256, a_l(l), 256, 256, true, &h));
        TRY(q.take_colsum(h, 0, 256, gr.pts_b[l]));
        TRY(q.take(h, 0, 0, 256, 256, l == 5 ? gr.pts_w[5] + PC + C : gr.pts_w[l], l == 5 ? ld5 : 256));
        if (l == 5) {
            TRY(q.product(w.dA[5], 256, 256, act(kActX0), 64, 64, false, &h));
            TRY(q.take(h, 0, 0, 256, PC, gr.pts_w[5], ld5));
        }
    }
    TRY(q.product(w.dA[0], 256, 256, act(kActX0), 64, 64, true, &h));
    TRY(q.take_colsum(h, 0, 256, gr.pts_b[0]));
    TRY(q.take(h, 0, 0, 256, PC, gr.pts_w[0], ld0));
    TRY(q.finish());
    const FoldBwdArgs f{p, cond.aud, cond.expr, cond.latent, gr.pts_b[0], gr.pts_b[5], gr.views_b[0], gr.pts_w[0], gr.pts_w[5],
                        gr.views_w[0], cond.d_aud, cond.d_latent, cond.d_expr};
    TRY(launch_fold_bwd(f, false, s));
#undef TRY
    return IDN_OK;
}

// d_x [n, pts_ch + views_ch] = dL / d (input rows) from the deltas of pts_linears.0 / .5 and views_linears.0 a backward has left in `w`
// (dx_kernel, below; launch_dx: idn_internal.h)

template <bool kNorm>
static void launch_composite_bwd_spl(const CompBwdArgs& a, hipStream_t s) {
    const dim3 grid((unsigned)((a.n_rays + 3) / 4)), block(256);
    switch ((a.S + 63) / 64) {
        case 1: hipLaunchKernelGGL((composite_bwd_kernel<1, kNorm>), grid, block, 0, s, a); break;
        case 2: hipLaunchKernelGGL((composite_bwd_kernel<2, kNorm>), grid, block, 0, s, a); break;
        case 3: hipLaunchKernelGGL((composite_bwd_kernel<3, kNorm>), grid, block, 0, s, a); break;
        case 4: hipLaunchKernelGGL((composite_bwd_kernel<4, kNorm>), grid, block, 0, s, a); break;
        case 5: hipLaunchKernelGGL((composite_bwd_kernel<5, kNorm>), grid, block, 0, s, a); break;
        case 6: hipLaunchKernelGGL((composite_bwd_kernel<6, kNorm>), grid, block, 0, s, a); break;
        case 7: hipLaunchKernelGGL((composite_bwd_kernel<7, kNorm>), grid, block, 0, s, a); break;
        default: hipLaunchKernelGGL((composite_bwd_kernel<8, kNorm>), grid, block, 0, s, a); break;
    }
}

// The compositing backward of a pass, and of idealnerf_composite_bwd: the bucket SPL = ceil(S / 64), the kNorm kernels where
// a.d_norm is given.
int launch_composite_bwd(const CompBwdArgs& a, hipStream_t s) {
    if (a.S < 2 || a.S > 64 * kMaxSpl) return fail(IDN_EUNSUPPORTED, "composite_bwd: n_samples %d outside [2, %d]", a.S, 64 * kMaxSpl);
    if (a.d_norm) launch_composite_bwd_spl<true>(a, s);
    else launch_composite_bwd_spl<false>(a, s);
    IDN_HIP_CHECK(hipGetLastError());
    return IDN_OK;
}

// d_rays != nullptr (idealnerf_pass_bwd_rays): after the backward, the input-row gradient of the pass's points (into the
// workspace: the delta matrix of pts_linears.1 is free once the weight gradients are reduced, and p_pad x 256 floats hold
// n x (pts_ch + views_ch <= 90)) and its reduction to the ray records (ray_grad.hip).  The compositing backward leaves dL / d |rays_d| in column 6
// of d_rays, which the reduction reads before it writes that column's zero.
int launch_pass_bwd(const PassBwd& b, hipStream_t s) {
    const idn_facenerf_params& p = *b.p;
    const int64_t n_rays = b.n_rays; const int S = b.S;
    float* const d_rays = b.d_rays;
    const int64_t P = n_rays * S;
    const int64_t Pp = (P + 127) / 128 * 128;
    if (S < 2 || S > 64 * kMaxSpl) return fail(IDN_EUNSUPPORTED, "pass_bwd: n_samples %d outside [2, %d]", S, 64 * kMaxSpl);
    const BwdWs w = carve_bwd(reinterpret_cast<char*>(b.ws), Pp);
    if (!b.ws || b.ws_bytes < w.bytes) return fail(IDN_EWORKSPACE, "backward workspace %zu < %zu", b.ws_bytes, w.bytes);

    // d(outputs) -> d raw, written straight into the head deltas (zero elsewhere)
    IDN_HIP_CHECK(hipMemsetAsync(w.dRGB, 0, (size_t)Pp * 64 * 4, s));
    // dV0: columns 0..127 are written by the delta chain for every row, column 128 (d sigma) by the compositing
    // backward for every real point; only the padding rows of that column need zeros.  Columns 129..255 are never written
    // here, but the views_linears.0 + alpha_linear product below READS all 256 columns: what it finds there is whatever an
    // earlier pass left in this workspace (the host layer hands over a workspace that was zeroed when it was allocated), and
    // it reaches only output rows / column sums 129..255, which `take` never asks for
    if (Pp > P) IDN_HIP_CHECK(hipMemsetAsync(w.dV0 + (size_t)P * 256, 0, (size_t)(Pp - P) * 256 * 4, s));
    {
        CompBwdArgs a{reinterpret_cast<const float4*>(b.raw), b.z, b.rays, b.bc, b.g_rgb, b.g_fg, b.g_lw, b.g_acc,
                      w.dRGB, 64, w.dV0 + kSigmaChannel, 256, (long)n_rays, S, d_rays ? d_rays + 6 : nullptr, IDN_RAY_FLOATS};
        if (int e = launch_composite_bwd(a, s)) return e;
    }
    if (int e = bwd_tail(p, b.grads, b.cond, b.acts, P, Pp, w, s)) return e;
    if (d_rays) {
        float* d_x = w.dA[1];
        static_assert(IDN_PTS_CH + IDN_VIEWS_CH <= 256, "the input-row gradient fits a delta matrix");
        if (int e = launch_dx(p, w.dA[0], w.dA[5], w.dV0, P, Pp, d_x, 0, nullptr, s)) return e;
        return launch_ray_grad(d_x, pts_ch_of(p), views_ch_of(p), b.rays, b.z, n_rays, S, d_rays, s);
    }
    return IDN_OK;
}

// ---------------------------------------------------------------------------
// FaceNeRF.forward's backward on pre-embedded rows (models/face_nerf.py:40-80): the head deltas come from the caller's
// d raw = g_out [n, 4] (rgb_raw, sigma_raw) instead of the compositing backward.  alpha_linear and rgb_linear are linear
// outputs, so d raw IS the head delta: one kernel writes dRGB (ld 64: columns 0..2, zeros beyond) and dV0 column
// kSigmaChannel for every row of the p_pad rows, zeros in the padding rows (they then carry zero deltas through the chain).
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(256) void head_seed_kernel(const float* g_out, long n, long p_pad, float* d_rgb, float* dv0) {
    const long idx = (long)blockIdx.x * 256 + threadIdx.x;   // (row, float4 of the 64-column dRGB row)
    const long p = idx >> 4;
    const int q = (int)(idx & 15);
    if (p >= p_pad) return;
    f32x4 v = {0.f, 0.f, 0.f, 0.f};
    if (q == 0 && p < n) v = f32x4{g_out[p * 4 + 0], g_out[p * 4 + 1], g_out[p * 4 + 2], 0.f};
    *reinterpret_cast<f32x4*>(d_rgb + p * 64 + 4 * q) = v;
    if (q == 0) dv0[p * 256 + kSigmaChannel] = p < n ? g_out[p * 4 + 3] : 0.f;
}

// ---------------------------------------------------------------------------
// Gradient with respect to the input rows x [n, 90] (rays never need it: their encoding is not a leaf):
//   d_x[:, 0:63]  = dA0 . W0[:, 0:63] + dA5 . W5[:, 0:63]     (pts_linears.0 and the skip layer, K = 512)
//   d_x[:, 63:90] = dV0[:, 0:128] . Wv0[:, 256:283]           (views_linears.0's direction columns, K = 128)
// (at the default widths; a narrower network has pts_ch / views_ch columns in place of 63 / 27 -- block-uniform run-time
// values: the fragments of the columns it does not have are zero, and the stores stop at its widths and use its row pitch)
// Row-major "NN" products, contraction over the layers' OUTPUT channels, on the fp32 matrix pipe (v_mfma_f32_32x32x2_f32,
// fp32 operands, fp32 accumulate).  One wave = 32 points: C[col][point] = W^T (A operand, from LDS) x delta^T (B operand,
// straight from the delta rows: lane (point j, half hh) loads the float4 of channels 8 g + 4 hh .. + 3 of its row and feeds
// them to four MFMAs; the A fragments hold the same four channels, so each delta row is read exactly once, as 16-byte loads).
// The three weight blocks are re-laid into fragment order in LDS once per (persistent) workgroup:
//   fragment 2 g + c (g < 64, c < 2): lane (i, hh) = W[k][32 c + i], k = 8 g + 4 hh + t, t = 0..3  (k < 256: W0 row k,
//                                      else W5 row k - 256; column 63 = 0)
//   fragment 128 + g (g < 16):         lane (i, hh) = Wv0[8 g + 4 hh + t][256 + i]  (i >= 27: 0)
// 144 fragments of 1 KiB: one 16-wave workgroup per CU.  DESIGN.md section 3 ("input gradient").
// ---------------------------------------------------------------------------
constexpr int kDxFrags = 2 * 64 + 16;
constexpr int kDxLds = kDxFrags * kFragBytes;
constexpr int kDxWaves = 16;
static_assert(kDxLds <= 160 * 1024, "the fragments must fit a CU's LDS");
struct DxArgs {
    const float* w0; int ld0;    // pts_linears.0.weight
    const float* w5; int ld5;    // pts_linears.5.weight
    const float* wv; int ldv;    // views_linears.0.weight
    const float* dA0; const float* dA5; const float* dV0;   // [p_pad, 256] deltas
    long n, p_pad;
    float* d_x;                  // [n, pts_ch + views_ch]
    int pts_ch, views_ch;        // the network's encoding widths (3..63, 3..27)
};
__global__ __launch_bounds__(64 * kDxWaves, 1) void dx_kernel(DxArgs a) {
    extern __shared__ __attribute__((aligned(16))) f32x4 dx_frag[];   // [kDxFrags][64 lanes]
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int j = lane & 31, hh = lane >> 5;
    for (int e = tid; e < kDxFrags * 64; e += 64 * kDxWaves) {
        const int f = e >> 6, i = e & 31, h = (e >> 5) & 1;
        float v[4];
        for (int t = 0; t < 4; ++t) {
            if (f < 128) {
                const int g = f >> 1, col = 32 * (f & 1) + i, k = 8 * g + 4 * h + t;
                const float* row = k < IDN_W ? a.w0 + (long)k * a.ld0 : a.w5 + (long)(k - IDN_W) * a.ld5;
                v[t] = col < a.pts_ch ? row[col] : 0.f;
            } else {
                const int k = 8 * (f - 128) + 4 * h + t;
                v[t] = i < a.views_ch ? a.wv[(long)k * a.ldv + IDN_W + i] : 0.f;
            }
        }
        dx_frag[e] = f32x4{v[0], v[1], v[2], v[3]};
    }
    __syncthreads();
    const long ntiles = a.p_pad / 32;
    for (long tile = (long)blockIdx.x * kDxWaves + wave; tile < ntiles; tile += (long)gridDim.x * kDxWaves) {
        const long p = tile * 32 + j;
        f32x16 acc0, acc1, accv;
        for (int r = 0; r < 16; ++r) acc0[r] = acc1[r] = accv[r] = 0.f;
        const float* r0 = a.dA0 + p * 256 + 4 * hh;
        const float* r5 = a.dA5 + p * 256 + 4 * hh;
        const float* rv = a.dV0 + p * 256 + 4 * hh;
#pragma unroll 4
        for (int g = 0; g < 32; ++g) {
            const f32x4 d = *reinterpret_cast<const f32x4*>(r0 + 8 * g);
            const f32x4 w0 = dx_frag[(2 * g) * 64 + lane], w1 = dx_frag[(2 * g + 1) * 64 + lane];
#pragma unroll
            for (int t = 0; t < 4; ++t) {
                acc0 = mfma32(w0[t], d[t], acc0);
                acc1 = mfma32(w1[t], d[t], acc1);
            }
        }
#pragma unroll 4
        for (int g = 0; g < 32; ++g) {
            const f32x4 d = *reinterpret_cast<const f32x4*>(r5 + 8 * g);
            const f32x4 w0 = dx_frag[(64 + 2 * g) * 64 + lane], w1 = dx_frag[(64 + 2 * g + 1) * 64 + lane];
#pragma unroll
            for (int t = 0; t < 4; ++t) {
                acc0 = mfma32(w0[t], d[t], acc0);
                acc1 = mfma32(w1[t], d[t], acc1);
            }
        }
#pragma unroll 4
        for (int g = 0; g < 16; ++g) {
            const f32x4 d = *reinterpret_cast<const f32x4*>(rv + 8 * g);
            const f32x4 w = dx_frag[(128 + g) * 64 + lane];
#pragma unroll
            for (int t = 0; t < 4; ++t) accv = mfma32(w[t], d[t], accv);
        }
        // lane (j, hh), register r: column d_row(r, hh) of point p (+ 32 for the second pts tile, + 63 for the direction block)
        if (p < a.n) {
            float* o = a.d_x + p * (a.pts_ch + a.views_ch);
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int col = d_row(r, hh);
                if (col < a.pts_ch) o[col] = acc0[r];   // (a network of fewer than 32 point columns ends inside the first tile)
                if (col < a.pts_ch - 32) o[32 + col] = acc1[r];
                if (col < a.views_ch) o[a.pts_ch + col] = accv[r];
            }
        }
    }
}

// max_blocks: 0 = the grid of a pass, min(ceil(Pp / 512), CUs); k > 0 caps it at k workgroups.  blocks_out (may be null): the grid that ran.
int launch_dx(const idn_facenerf_params& p, const float* dA0, const float* dA5, const float* dV0, int64_t n, int64_t Pp, float* d_x,
              int max_blocks, int* blocks_out, hipStream_t s) {
    static LaunchSetup setup;
    int num_cu = 0;
    if (int e = setup.get([]() -> int {
            IDN_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(&dx_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, kDxLds));
            return IDN_OK;
        }, &num_cu))
        return e;
    const int C = p.dim_aud + p.dim_expr + p.dim_latent;
    const int PC = pts_ch_of(p), VC = views_ch_of(p);
    const DxArgs da{p.pts_w[0], PC + C, p.pts_w[5], PC + C + IDN_W, p.views_w[0], IDN_W + VC + p.dim_expr,
                    dA0, dA5, dV0, (long)n, (long)Pp, d_x, PC, VC};
    const int64_t groups = (Pp / 32 + kDxWaves - 1) / kDxWaves;
    int grid = (int)(groups < num_cu ? groups : num_cu);
    if (max_blocks > 0 && grid > max_blocks) grid = max_blocks;
    hipLaunchKernelGGL(dx_kernel, dim3(grid), dim3(64 * kDxWaves), kDxLds, s, da);
    IDN_HIP_CHECK(hipGetLastError());
    if (blocks_out) *blocks_out = grid;
    return IDN_OK;
}

int launch_facenerf_bwd(const idn_facenerf_params& p, const idn_facenerf_grads& gr, const BwdCond& cond, const float* acts,
                        int64_t n, const float* g_out, float* d_x, void* ws_, size_t ws_bytes, hipStream_t s) {
    const int64_t Pp = (n + 127) / 128 * 128;
    const BwdWs w = carve_bwd(reinterpret_cast<char*>(ws_), Pp);
    if (!ws_ || ws_bytes < w.bytes) return fail(IDN_EWORKSPACE, "backward workspace %zu < %zu", ws_bytes, w.bytes);
    {
        const long threads = (long)Pp * 16;
        hipLaunchKernelGGL(head_seed_kernel, dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, s, g_out, (long)n, (long)Pp,
                           w.dRGB, w.dV0);
        IDN_HIP_CHECK(hipGetLastError());
    }
    if (int e = bwd_tail(p, &gr, cond, acts, n, Pp, w, s)) return e;
    if (d_x) return launch_dx(p, w.dA[0], w.dA[5], w.dV0, n, Pp, d_x, 0, nullptr, s);
    return IDN_OK;
}

}  // namespace idn
