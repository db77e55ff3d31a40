// The weight-gradient (dW) products of the training backward: dW = delta^T . acts, contraction over the points, as partial
// blocks per split of the points (dw_gemm.hip: gemm_tn_kernel on the fp32 matrix pipe, gemm_tn_x6_kernel as six bf16 piece
// products) that one reduction launch sums into the gradient tensors.  DwPass schedules the products of one backward pass.
#pragma once
#include "mlp_common.h"

namespace idn {

__device__ __forceinline__ f32x16 mfma32(float a, float b, f32x16 c) { return __builtin_amdgcn_mfma_f32_32x32x2f32(a, b, c, 0, 0, 0); }
__device__ __forceinline__ int d_row(int r, int hh) { return (r & 3) + 8 * (r >> 2) + 4 * hh; }   // (both: dx_kernel too, train.hip)

// ---------------------------------------------------------------------------
// TN GEMM: part[split][n][k] = sum_{p in split} A[p][n0+n] * B[p][k0+k]
// Block = (64*NTW) x (64*KTW) outputs, waves 2 x 2, contraction chunk 32 points.
// ---------------------------------------------------------------------------
struct TNArgs {
    const float* A; int lda;   // delta  [P, >= N]
    const float* B; int ldb;   // acts   [P, >= K]
    float* part;               // [splits][N][K]
    int N, K;
    long P;                    // rows (multiple of 32)
    int chunks_per_split;      // kTnRows-row chunks per split
    float* cpart;              // optional [splits][N]: column sums of A (the bias gradient), from the k-block-0 workgroups
    // gemm_tn_x6_kernel only: B as TWO 128-column matrices (row pitch ldb each), columns 0..127 at B + b_off0 bytes and
    // columns 128..255 at B + b_off1 bytes -- two 128 x 128 products as the diagonal blocks of one 256 x 256 launch
    int b_split, b_off0, b_off1;
    // (skipping the MFMAs of the unwanted tiles -- the off-diagonal blocks of a paired launch, rows 129..255 of views_linears.0 +
    //  alpha_linear -- behind wave-uniform branches was tried: the accumulators then flow through phis, hipcc copies registers whose
    //  asm loads are in flight (556 sites in tools/audit_asm_loads.py, results no longer reproducible) and the kernel ran 1.6x slower)
};
constexpr int kMaxTnBatch = 12;
struct TNBatch {
    TNArgs it[kMaxTnBatch];
    int n, splits;
};
constexpr int kMaxReduceItems = 32;
struct ReduceItem {
    const float* part;   // [splits][N][K], already offset to the first row / column wanted
    float* out;
    int splits, N, K, ldo, rows, cols;
    int block_end;       // exclusive end of this item's block range
};
struct ReduceBatch {
    ReduceItem it[kMaxReduceItems];
    int n;
};

inline size_t al256(size_t x) { return (x + 255) & ~(size_t)255; }
// which matrix pipe a 256 x 256 product runs on (the other shapes: fp32)
enum { kPipeX6 = IDN_DW_PIPE_BF16X6, kPipeF32 = IDN_DW_PIPE_F32 };

// The products of one training pass (bwd_tail, train.hip), in its order.  pipes: bit kPipeX6 / kPipeF32 = that pipe's pass has it
struct DwPassProduct { int N, K; bool colsum; int pipes; };
constexpr int kOnX6 = 1 << kPipeX6, kOnF32 = 1 << kPipeF32, kOnBoth = kOnX6 | kOnF32;
constexpr DwPassProduct kTrunk = {256, 256, true, kOnBoth};
constexpr DwPassProduct kPassProducts[] = {
    {64, 128, true, kOnBoth},                                                            // rgb_linear
    {256, 256, true, kOnX6}, {128, 128, true, kOnF32}, {128, 128, true, kOnF32},         // views_linears.2 | .1: one product on the x6 pipe, two on the fp32 pipe
    kTrunk, {128, 64, false, kOnBoth},                                                   // views_linears.0 + alpha_linear; its direction columns
    kTrunk, kTrunk, kTrunk, {256, 64, false, kOnBoth}, kTrunk, kTrunk, kTrunk, kTrunk,   // pts_linears.7 .. .1, behind .5 its encoding columns
    {256, 64, true, kOnBoth},                                                            // pts_linears.0
};
// summed over a pipe's pass: 0 = its 256 x 256 products, 1 / 2 = the floats ONE split adds to the partial-block / column-sum pool
constexpr size_t pass_sum(int pipe, int what) {
    size_t n = 0;
    for (const DwPassProduct& t : kPassProducts)
        if (t.pipes >> pipe & 1) n += what == 0 ? (t.N == 256 && t.K == 256) : what == 1 ? (size_t)t.N * t.K : t.colsum ? t.N : 0;
    return n;
}
// the x6 pipe's 256 x 256 products go out as ONE launch, the CUs divided among them
constexpr int kX6ItemsPerPass = (int)pass_sum(kPipeX6, 0);
static_assert(kX6ItemsPerPass == 9 && kX6ItemsPerPass <= kMaxTnBatch, "one x6 batch per pass");

// The pools of the backward workspace (carve_bwd, train.hip).  No product runs more than kMaxSplits splits (the shape table of
// dw_gemm.hip), so a pass fits if one split of it does; DwPass::product checks every slab against the pools all the same.
constexpr int kMaxSplits = 256;
constexpr int kColsumBlocks = 256;   // rows of the column-sum partial buffer (>= kMaxSplits)
constexpr int kGemmsPerPass = 16;
constexpr size_t kPartFloatsPerSplit = 9 * 65536 + 6 * 16384 + 4 * 8192;
constexpr size_t kPartPoolFloats = (size_t)kMaxSplits * kPartFloatsPerSplit, kCpartPoolFloats = (size_t)kColsumBlocks * 256 * kGemmsPerPass;
static_assert(pass_sum(kPipeX6, 1) <= kPartFloatsPerSplit && pass_sum(kPipeF32, 1) <= kPartFloatsPerSplit, "a pass's partial blocks fit");
static_assert(kMaxSplits * pass_sum(kPipeX6, 2) <= kCpartPoolFloats && kMaxSplits * pass_sum(kPipeF32, 2) <= kCpartPoolFloats, "a pass's column sums fit");

// where a product's partial blocks went: part [splits][N][K], cpart [splits][N] or null; chunks_per_split: what its kernel was given
struct DwProduct { const float *part, *cpart; int splits, N, K, chunks_per_split; };

// The dW products of ONE backward pass over P rows: fp32 products launch as they are named, the 256 x 256 bf16-piece products
// and every reduction are queued; finish() launches the x6 batch, then one reduce_batch_kernel.  Fixed-size, on the stack.
struct DwPass {
    // x6_items: how many 256 x 256 bf16-piece products the caller will name (the CUs are divided among them)
    DwPass(float* part, size_t part_floats, float* cpart, size_t cpart_floats, int64_t P, int pipe, int x6_items, hipStream_t s)
        : part_next(part), part_left(part_floats), cpart_next(cpart), cpart_left(cpart_floats), P(P), pipe(pipe), x6_items(x6_items), s(s) {}
    // partial blocks of A[:, :N]^T . B[:, :K] into the next slab of the pools (want_colsum: and the column sums of A).
    // B2: the x6 kernel's split-B form (two 128-column matrices, B for output columns 0..127 and B2 for 128..255)
    int product(const float* A, int lda, int N, const float* B, int ldb, int K, bool want_colsum, DwProduct* h, const float* B2 = nullptr);
    // out[(0..rows) x (0..cols)] (ld ldo) = sum over the splits of the product's blocks, from row row0 / column col0 on
    int take(const DwProduct& h, int row0, int col0, int rows, int cols, float* out, int ldo);
    int take_colsum(const DwProduct& h, int col0, int cols, float* out);
    int finish();

private:
    float* part_next; size_t part_left;   // what is left of the two pools
    float* cpart_next; size_t cpart_left;
    int64_t P;
    int pipe, x6_items;
    hipStream_t s;
    TNBatch x6{{}, 0, 0};   // the 256 x 256 bf16-piece products named so far
    ReduceBatch red{{}, 0};
    int red_blocks = 0;
};

}  // namespace idn
