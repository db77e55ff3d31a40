// Frame scores on the device (gfx950): squared error and SSIM of a rendered fp32 frame against its uint8 ground truth, whole frame
// and per sampling region (include/idealnerf.h: idealnerf_frame_scores).  PSNR is the reference's (NeRFs/HeadNeRF/helper.py:151,
// mse2psnr of img2mse against target = uint8 / 255); SSIM is Wang et al. 2004 with the 11 x 11 sigma-1.5 window.
//
//   frame_scores_tiles:  one workgroup per kTile x kTile tile.  It owns the tile's PIXELS (squared error) and the windows whose
//                        top-left corner lies in the tile (SSIM), so it stages a (kTile + 10)^2 halo tile of one channel of both
//                        images in LDS, filters it along the rows into five fp64 moment planes (x, t, x x, t t, x t) and then along
//                        the columns; the SSIM expression is fp64 too.  E[x x] - mu^2 cancels against C2 = 9e-4: fp32 window sums
//                        move single windows by 3e-4, fp64 ones by 1e-12.
//   frame_scores_final:  the workgroups' 20 partial sums, added in workgroup order.
//
// No floating-point atomics anywhere: every lane adds its items in a fixed order, a wave folds its lanes by a fixed shuffle tree,
// the waves of a workgroup and the workgroups of a frame are added in index order.  The 160 bytes of `out` depend on the inputs alone.
#include "idn_internal.h"

namespace idn {

constexpr int kTile = IDN_SCORE_TILE;
constexpr int kWin = 11;
constexpr int kHalo = kTile + kWin - 1;          // 42
constexpr int kScoreThreads = 256;
constexpr int kScoreWaves = kScoreThreads / 64;
constexpr int kGroups = 5, kCols = 4;            // rows and columns of `out`
constexpr int kSums = kGroups * kCols;
static_assert(kTile == 32, "the row and column filters index a tile row as idx & 31");

// exp(-(k - 5)^2 / (2 * 1.5^2)), k = 0..10, normalised in fp64 and rounded to fp32
__constant__ const float kGauss[kWin] = {0.00102838012f, 0.00759875821f, 0.0360007733f, 0.109360687f, 0.213005543f, 0.266011715f,
                                         0.213005543f,   0.109360687f,   0.0360007733f, 0.00759875821f, 0.00102838012f};

__global__ __launch_bounds__(kScoreThreads) void frame_scores_tiles(const float* __restrict__ pred, const unsigned char* __restrict__ truth,
                                                                    const unsigned char* __restrict__ regions, int H, int W, int tiles_x,
                                                                    double* __restrict__ partial) {
    __shared__ double hm[5][kHalo][kTile];        // row-filtered moments, 52.5 KiB
    __shared__ float sx[kHalo][kHalo];            // prediction, one channel
    __shared__ unsigned char st[kHalo][kHalo];    // truth, one channel, as bytes: 64 KiB of static LDS hold no second fp32 tile
    __shared__ float unit[256];                   // byte -> fp32(byte) / 255.0f
    __shared__ double red[kScoreWaves][kSums];
    static_assert(sizeof(double) * 5 * kHalo * kTile + 5 * kHalo * kHalo + 1024 + sizeof(double) * kScoreWaves * kSums <= 65536,
                  "static LDS of one workgroup");

    const int tid = threadIdx.x;
    const int y0 = (int)(blockIdx.x / (unsigned)tiles_x) * kTile, x0 = (int)(blockIdx.x % (unsigned)tiles_x) * kTile;
    const bool windows = y0 + kWin <= H && x0 + kWin <= W;   // the tile's first window fits (false for every tile when H or W < 11)

    unit[tid] = (float)tid / 255.0f;              // read behind the first barrier
    static_assert(kScoreThreads == 256, "one thread per byte value");

    double acc[kGroups][kCols];
#pragma unroll
    for (int g = 0; g < kGroups; ++g)
#pragma unroll
        for (int c = 0; c < kCols; ++c) acc[g][c] = 0.0;

    for (int ch = 0; ch < 3; ++ch) {
        // ---- stage the halo tile; the tile's own pixels add their squared error on the way
        for (int idx = tid; idx < kHalo * kHalo; idx += kScoreThreads) {
            const int r = idx / kHalo, c = idx - r * kHalo;
            const int y = y0 + r, x = x0 + c;
            float xv = 0.0f;
            unsigned char tb = 0;
            if (y < H && x < W) {
                const size_t pix = (size_t)y * (size_t)W + (size_t)x;
                xv = pred[pix * 3 + ch];
                tb = truth[pix * 3 + ch];
                const float tv = (float)tb / 255.0f;
                if (r < kTile && c < kTile) {
                    const float d = xv - tv;
                    const double e = (double)(d * d);
                    const unsigned m = 1u | (regions ? ((unsigned)regions[pix] & 15u) << 1 : 0u);
#pragma unroll
                    for (int g = 0; g < kGroups; ++g)
                        if ((m >> g) & 1u) {
                            if (ch == 0) acc[g][0] += 1.0;
                            acc[g][1] += e;
                        }
                }
            }
            sx[r][c] = xv;
            st[r][c] = tb;
        }
        if (!windows) continue;   // uniform over the workgroup: no barrier is skipped by a part of it
        __syncthreads();
        // ---- along the rows: hm[.][r][c] = sum_k w[k] f(r, c + k)
        for (int idx = tid; idx < kHalo * kTile; idx += kScoreThreads) {
            const int r = idx >> 5, c = idx & 31;
            double a = 0.0, b = 0.0, aa = 0.0, bb = 0.0, ab = 0.0;
#pragma unroll
            for (int k = 0; k < kWin; ++k) {
                const double w = (double)kGauss[k], xv = (double)sx[r][c + k], tv = (double)unit[st[r][c + k]];
                a += w * xv;
                b += w * tv;
                aa += w * (xv * xv);
                bb += w * (tv * tv);
                ab += w * (xv * tv);
            }
            hm[0][r][c] = a; hm[1][r][c] = b; hm[2][r][c] = aa; hm[3][r][c] = bb; hm[4][r][c] = ab;
        }
        __syncthreads();
        // ---- along the columns, then the index of window (y0 + r, x0 + c): rows y0 + r .. + 10, columns x0 + c .. + 10
        for (int idx = tid; idx < kTile * kTile; idx += kScoreThreads) {
            const int r = idx >> 5, c = idx & 31;
            const int y = y0 + r, x = x0 + c;
            if (y + kWin > H || x + kWin > W) continue;
            double mo[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
#pragma unroll
            for (int k = 0; k < kWin; ++k) {
                const double w = (double)kGauss[k];
#pragma unroll
                for (int q = 0; q < 5; ++q) mo[q] += w * hm[q][r + k][c];
            }
            const double C1 = 1e-4, C2 = 9e-4;
            const double mx = mo[0], mt = mo[1];
            const double vx = mo[2] - mx * mx, vt = mo[3] - mt * mt, cov = mo[4] - mx * mt;
            const double ssim = ((2.0 * mx * mt + C1) * (2.0 * cov + C2)) / ((mx * mx + mt * mt + C1) * (vx + vt + C2));
            const size_t centre = (size_t)(y + kWin / 2) * (size_t)W + (size_t)(x + kWin / 2);
            const unsigned m = 1u | (regions ? ((unsigned)regions[centre] & 15u) << 1 : 0u);
#pragma unroll
            for (int g = 0; g < kGroups; ++g)
                if ((m >> g) & 1u) {
                    if (ch == 0) acc[g][2] += 1.0;
                    acc[g][3] += ssim;
                }
        }
        // the next channel's staging writes sx / st, last read before the barrier above; its row filter writes hm behind its own barrier
    }

    // ---- lanes -> wave (shuffle tree) -> workgroup (waves in order)
#pragma unroll
    for (int g = 0; g < kGroups; ++g)
#pragma unroll
        for (int c = 0; c < kCols; ++c) {
            double v = acc[g][c];
#pragma unroll
            for (int d = 32; d > 0; d >>= 1) v += __shfl_down(v, d, 64);
            if ((tid & 63) == 0) red[tid >> 6][g * kCols + c] = v;
        }
    __syncthreads();
    if (tid < kSums) {
        double v = red[0][tid];
#pragma unroll
        for (int w = 1; w < kScoreWaves; ++w) v += red[w][tid];
        partial[(size_t)blockIdx.x * kSums + tid] = v;
    }
}

__global__ __launch_bounds__(64) void frame_scores_final(const double* __restrict__ partial, int n_tiles, double* __restrict__ out) {
    const int tid = threadIdx.x;
    if (tid >= kSums) return;
    double v = 0.0;
#pragma unroll 8
    for (int b = 0; b < n_tiles; ++b) v += partial[(size_t)b * kSums + tid];
    out[tid] = v;
}

static int score_tiles(int H, int W) { return ((H + kTile - 1) / kTile) * ((W + kTile - 1) / kTile); }

size_t frame_scores_workspace_bytes(int H, int W) {
    if (H <= 0 || W <= 0) return 0;
    return (size_t)score_tiles(H, W) * kSums * sizeof(double);
}

int launch_frame_scores(const float* pred, const unsigned char* truth, const unsigned char* regions, int H, int W, double* out,
                        double* partial, hipStream_t s) {
    const int tiles_x = (W + kTile - 1) / kTile, n_tiles = score_tiles(H, W);
    hipLaunchKernelGGL(frame_scores_tiles, dim3((unsigned)n_tiles), dim3(kScoreThreads), 0, s, pred, truth, regions, H, W, tiles_x, partial);
    IDN_HIP_CHECK(hipGetLastError());
    hipLaunchKernelGGL(frame_scores_final, dim3(1), dim3(64), 0, s, (const double*)partial, n_tiles, out);
    IDN_HIP_CHECK(hipGetLastError());
    return IDN_OK;
}

}  // namespace idn
