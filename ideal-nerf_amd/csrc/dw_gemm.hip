// The weight-gradient (dW) products of the training backward (dw_gemm.h): gemm_tn_kernel (fp32 MFMA), gemm_tn_x6_kernel (the
// 256 x 256 ones of a pass as six bf16 piece products, one launch), reduce_batch_kernel (sums the per-split blocks of all layers
// into the gradient tensors, one launch per pass) and DwPass, which schedules them.  gfx950.  Deterministic: no float atomics.
#include "dw_gemm.h"
#include "mlp_x6.h"

namespace idn {

// The two 32-row chunk tiles are double-buffered in LDS and filled by LDS-DMA (a chunk row is
// contiguous in global memory and in the tile, so one wave instruction moves 1 KiB of it): the
// loads of chunk c+1 are in flight while chunk c is multiplied, one barrier per chunk.  (Single
// buffered, every chunk paid its global-load latency: 70 % of the fp32 MFMA peak.)
//
// Operand reads.  MFMA row i of a wave's tile x is output channel NTW * i + x (not 32 x + i): a lane's NTW
// A values of one point are then CONTIGUOUS in the row-major LDS tile and come with one ds_read_b128
// (b64 / b32) instead of NTW strided ds_read_b32; the same for B.  The reads of point-pair s + 1 are
// issued before the MFMAs of pair s from inline asm and retired by a counted wait tied to the
// destination registers (hipcc issues such reads right before their use and waits lgkmcnt(0): an exposed
// LDS round trip every 8 MFMAs, 12 % of the wave cycles parked, measured with SQ_WAIT_ANY).
template <int N>
struct LdsVec;
template <>
struct LdsVec<4> {
    f32x4 v;
    template <int OFF>
    __device__ __forceinline__ void issue(uint32_t addr) { asm volatile("ds_read_b128 %0, %1 offset:%2" : "=v"(v) : "v"(addr), "n"(OFF) : "memory"); }
    __device__ __forceinline__ float get(int j) const { return v[j]; }
};
template <>
struct LdsVec<2> {
    typedef float f32x2 __attribute__((ext_vector_type(2)));
    f32x2 v;
    template <int OFF>
    __device__ __forceinline__ void issue(uint32_t addr) { asm volatile("ds_read_b64 %0, %1 offset:%2" : "=v"(v) : "v"(addr), "n"(OFF) : "memory"); }
    __device__ __forceinline__ float get(int j) const { return v[j]; }
};
template <>
struct LdsVec<1> {
    float v;
    template <int OFF>
    __device__ __forceinline__ void issue(uint32_t addr) { asm volatile("ds_read_b32 %0, %1 offset:%2" : "=v"(v) : "v"(addr), "n"(OFF) : "memory"); }
    __device__ __forceinline__ float get(int) const { return v; }
};
template <int OFF>
__device__ __forceinline__ void lds_read_f32(float& dst, uint32_t addr) {
    asm volatile("ds_read_b32 %0, %1 offset:%2" : "=v"(dst) : "v"(addr), "n"(OFF) : "memory");
}
// use of an asm-read value: not before the counted wait that precedes this call in program order
__device__ __forceinline__ float landed(float& v) {
    asm volatile("" : "+v"(v));
    return v;
}
// all but the newest `NEWER` LDS reads of this wave have completed => a, b are valid
template <int NEWER, class VA, class VB>
__device__ __forceinline__ void lds_retire(VA& a, VB& b) {
    if constexpr (NEWER == 0) asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(a.v), "+v"(b.v)::"memory");
    else asm volatile("s_waitcnt lgkmcnt(2)" : "+v"(a.v), "+v"(b.v)::"memory");
}

// Chunks of kTnRows points; kTnBufs LDS buffers: while chunk c is multiplied, the pieces of chunk c + 2 are
// issued ONE PER POINT-PAIR STEP (a burst of 16 LDS-DMA instructions at the top of a chunk held the wave's
// MFMA issue for ~10 % of the chunk), as `buffer_load ... lds` with a per-lane constant offset and a scalar
// row offset (half the issue cost of the per-lane-pointer form), and they have a whole chunk to land: the
// GEMM reads 2 KiB per point and layer for 131 kFLOP, i.e. it needs 2.5 TB/s of HBM at the MFMA peak.
constexpr int kTnRows = 16, kTnBufs = 3;
// The narrow shapes (256 x 64, 128 x 64, 64 x 128 outputs: pts_linears.0, the encoding columns of pts_linears.5, the direction
// columns of views_linears.0, rgb_linear) are HBM-shaped: ring depth and workgroups per CU decide how many bytes they keep in flight
constexpr int kTnNarrowBufs = 3;
// points per chunk of the narrow shapes: 256 x 64 (40 KiB per 32-point chunk) and 128 x 64 / 64 x 128 (48 KiB per 64-point chunk)
constexpr int kTnRows4x1 = 32, kTnRowsThin = 64;
constexpr int kTnNarrowSplits = 256;

// NB = LDS buffers of the chunk ring: the pieces of chunk c + NB - 1 are issued while chunk c is multiplied.  The 256 x 256
// shape (32 KiB per chunk, 16 MFMAs per point pair and wave) runs NB = 3; the narrow shapes do a quarter of the arithmetic per
// byte (a 256 x 64 chunk is 20 KiB for 4 MFMAs per point pair: 1 us of matrix time, less than a loaded HBM round trip) and
// run a deeper ring, so that several chunks per workgroup are in flight.
// R = points per chunk (a multiple of 16).  A chunk costs ~1 000 cycles besides its MFMAs (the barrier and its skew, the first LDS
// reads behind it with nothing to overlap, the drain of the prefetched reads at its end: in-kernel stamps, profiles/r04_diag_tn_4x1.log:
// 3 007 cycles per 16-point chunk of the 256 x 64 shape against 2 048 of MFMAs), so the shapes with few MFMAs per point take
// larger chunks.
template <int NTW, int KTW, int NB = kTnBufs, int R = kTnRows>
__global__ __launch_bounds__(256) void gemm_tn_kernel(TNArgs g) {
    static_assert(R % 16 == 0, "chunks are multiples of 16 points");
    constexpr int NPA = NTW * R / 16, NPB = KTW * R / 16;   // 1-KiB pieces of the A / B tile per wave and chunk
    static_assert(NB >= 3 && (NB - 2) * (NPA + NPB) <= 63, "vmcnt is a 6-bit field");
    constexpr int BN = 64 * NTW, BK = 64 * KTW;
    constexpr int kTileFloats = R * (BN + BK);       // one chunk: A tile then B tile
    constexpr int kSteps = R / 2;                    // point-pairs per chunk
    constexpr int NP = NPA + NPB;                          // 1-KiB pieces per wave and chunk (<= kSteps)
    static_assert(NP <= kSteps, "at most one piece per step");
    extern __shared__ __attribute__((aligned(16))) float tn_smem[];  // NB * kTileFloats
    const int tid = threadIdx.x, lane = tid & 63;
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int i = lane & 31, hh = lane >> 5;
    const int wr = w >> 1, wc = w & 1;
    const int n0 = blockIdx.x * BN, k0 = blockIdx.y * BK;
    const int split = blockIdx.z;
    f32x16 acc[NTW][KTW];
#pragma unroll
    for (int a = 0; a < NTW; ++a)
#pragma unroll
        for (int b = 0; b < KTW; ++b)
            for (int r = 0; r < 16; ++r) acc[a][b][r] = 0.f;

    const long c_begin = (long)split * g.chunks_per_split;
    long c_end = c_begin + g.chunks_per_split;
    const long c_total = g.P / R;
    if (c_end > c_total) c_end = c_total;
    const bool colsum_block = g.cpart != nullptr && blockIdx.y == 0;   // block-uniform
    const bool do_colsum = colsum_block && tid < BN;
    const int ccol = tid < BN ? tid : 0;                                  // threads beyond the tile re-read column 0 (unused)
    float csum = 0.0f;

    // A piece = 256 consecutive floats of a tile = 256 / BN rows of it.  Piece j (0 .. NTW-1) of wave w is
    // tile piece NTW * w + j: rows (NTW * w + j) * (256 / BN) ..; lane l moves float4 l of the piece.
    constexpr int kRowsPerPieceA = 256 / BN > 0 ? 256 / BN : 1, kRowsPerPieceB = 256 / BK > 0 ? 256 / BK : 1;
    // descriptors based at this block's first row: the 32-bit piece offsets then span one split (tens of MB), not the
    // whole matrix (which passes 4 GB from 4 M points on)
    const __amdgpu_buffer_rsrc_t rsrcA = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(g.A + n0 + c_begin * R * (long)g.lda), 0, 0xfffffffc, 0x00020000);
    const __amdgpu_buffer_rsrc_t rsrcB = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(g.B + k0 + c_begin * R * (long)g.ldb), 0, 0xfffffffc, 0x00020000);
    const uint32_t voffA = ((lane / (BN / 4)) * g.lda + (lane % (BN / 4)) * 4) * 4;
    const uint32_t voffB = ((lane / (BK / 4)) * g.ldb + (lane % (BK / 4)) * 4) * 4;
    const uint32_t rowA = g.lda * 4, rowB = g.ldb * 4;    // bytes per matrix row
    // piece ja (0 .. NTW-1) of this wave's share of the A tile / piece jb (0 .. KTW-1) of the B tile, for chunk c
    // into buffer `buf`: scalar arithmetic only (a piece that had to choose between the two matrices cost a
    // tree of scalar branches per point pair, ~10 % of the loop)
    auto piece_a = [&](long c, int buf, int ja) {
        const int pc = NPA * w + ja;
        __builtin_amdgcn_raw_ptr_buffer_load_lds(rsrcA, (__attribute__((address_space(3))) void*)(tn_smem + buf * kTileFloats + pc * 256), 16, voffA,
                                                 (uint32_t)(((c - c_begin) * R + pc * kRowsPerPieceA) * rowA), 0, 0);
    };
    auto piece_b = [&](long c, int buf, int jb) {
        const int pc = NPB * w + jb;
        __builtin_amdgcn_raw_ptr_buffer_load_lds(rsrcB, (__attribute__((address_space(3))) void*)(tn_smem + buf * kTileFloats + R * BN + pc * 256), 16, voffB,
                                                 (uint32_t)(((c - c_begin) * R + pc * kRowsPerPieceB) * rowB), 0, 0);
    };
    auto piece = [&](long c, int buf, int j) {   // prologue order: A pieces, then B pieces
        if (j < NPA) piece_a(c, buf, j);
        else if (j < NP) piece_b(c, buf, j - NPA);
    };
    // LDS byte addresses of this lane's operands of point-pair 0 in buffer 0: row hh, columns NTW * (32 wr + i) ..
    const uint32_t smem0 = (uint32_t)(uintptr_t)(__attribute__((address_space(3))) float*)tn_smem;
    const uint32_t a_addr0 = smem0 + (hh * BN + NTW * (32 * wr + i)) * 4;
    const uint32_t b_addr0 = smem0 + (R * BN + hh * BK + KTW * (32 * wc + i)) * 4;
    // every chunk's NP pieces are issued even past the end of the split (clamped to its last chunk: re-read, never used), so
    // that exactly (NB - 2) * NP younger vector-memory operations are in flight at every chunk's wait
    for (int ahead = 0; ahead < NB - 1; ++ahead)
        for (int j = 0; j < NP; ++j) piece(c_begin + ahead < c_end ? c_begin + ahead : c_end - 1, ahead, j);
    int buf = 0;
    for (long c = c_begin; c < c_end; ++c) {
        // this wave's pieces of chunk c have landed (those of chunks c + 1 .. c + NB - 2, issued later, may still be in flight)
        asm volatile("s_waitcnt vmcnt(%0)" ::"n"((NB - 2) * NP) : "memory");
        // everyone's have; everyone is done with chunk c - 1, whose buffer chunk c + 2 now takes.  A raw barrier:
        // __syncthreads() would add its own vmcnt(0) and wait for the pieces of chunk c + 1 as well
        __builtin_amdgcn_s_barrier();
        asm volatile("" ::: "memory");
        const int buf2 = buf >= 1 ? buf - 1 : NB - 1;   // (buf + NB - 1) % NB: the buffer chunk c - 1 has just left
        const long cnext = c + NB - 1 < c_end ? c + NB - 1 : c_end - 1;   // clamped: the re-read of the last chunk is never used
        // The delta tile is in LDS anyway: its column sums are the bias gradient.  The R reads of column
        // `tid` go out first (inline asm, like the operand reads) and are added after the first counted wait of
        // the loop below, which covers them (LDS returns in order): read by plain loads they parked every wave
        // for two LDS round trips per chunk, 5 % of it.
        // (In batches of 16 rows: batch k + 1 is issued at the end of loop iteration k -- in front of that iteration's operand
        // reads, whose counted wait in iteration k + 1 then covers it -- into the registers batch k has just been added from.)
        float cs[16];
        auto cs_issue = [&](int batch) {
            const uint32_t caddr = smem0 + buf * (kTileFloats * 4) + ccol * 4 + batch * (16 * BN * 4);
            static_for<16>([&](auto Row) {
                lds_read_f32<decltype(Row)::value * BN * 4>(cs[decltype(Row)::value], caddr);
            });
        };
        static_assert(R / 16 <= kSteps / 4, "one batch of column reads per iteration of the first half loop");
        if (colsum_block) cs_issue(0);
        // kSteps point-pairs, two per loop iteration (one per register buffer); the loop is kept rolled: fully
        // unrolled, hipcc shuffles the 256 accumulator registers between steps (~500 v_accvgpr_mov per chunk)
        LdsVec<NTW> a0v, a1v;
        LdsVec<KTW> b0v, b1v;
        constexpr int kStepA = 2 * BN * 4, kStepB = 2 * BK * 4;   // bytes from one point-pair to the next
        uint32_t pa = a_addr0 + buf * (kTileFloats * 4), pb = b_addr0 + buf * (kTileFloats * 4);
        a0v.template issue<0>(pa);
        b0v.template issue<0>(pb);
        // first half of the chunk: the A pieces of chunk c + 2 (one per point pair), second half: its B pieces
        static_assert(NPA <= kSteps / 2 && NPB <= kSteps / 2, "pieces of one matrix fit one half of a chunk");
        constexpr int M = NTW * KTW;        // MFMAs per point pair
        if constexpr (M >= 4) {
            // The fp32 MFMA issues every 64 cycles and everything else issues IN ORDER between two of them: left to hipcc, a
            // pair's MFMAs go out back to back and its ~20 other instructions (operand reads, the LDS-DMA piece with its scalar
            // address arithmetic, pointer updates, the loop branch) follow in one run -- longer than the 60 cycles the last MFMA
            // leaves free, so the matrix pipe idled ~120 cycles per point pair (in-kernel stamps: 376 cycles per pair of the
            // 256 x 64 shape against 256; the same ~120 on the 1 024 of the 256 x 256 shape).  The other work is therefore cut into
            // three slots placed behind the first three MFMAs of a pair, with scheduling fences; the pair's operands are read in
            // the shadow of the pair before (three MFMAs = 190 cycles ahead of their first use).
            auto step = [&](LdsVec<NTW>& ca, LdsVec<KTW>& cb, auto&& side0, auto&& side1, auto&& side2) {
                lds_retire<0>(ca, cb);
                static_for<M>([&](auto M_) {
                    constexpr int m = decltype(M_)::value, x = m / KTW, y = m % KTW;
                    acc[x][y] = mfma32(ca.get(x), cb.get(y), acc[x][y]);
                    if constexpr (m < 3) {
                        __builtin_amdgcn_sched_barrier(0);
                        if constexpr (m == 0) side0();
                        if constexpr (m == 1) side1();
                        if constexpr (m == 2) side2();
                        __builtin_amdgcn_sched_barrier(0);
                    }
                });
            };
#pragma unroll 1
            for (int it = 0; it < kSteps / 4; ++it) {
                step(a0v, b0v,
                     [&]() { a1v.template issue<kStepA>(pa); b1v.template issue<kStepB>(pb); },
                     [&]() { if (2 * it < NPA) piece_a(cnext, buf2, 2 * it); },
                     [&]() {
                         if (colsum_block && it < R / 16) {   // batch `it` of the column reads is older than a0v / b0v: retired with them
                             static_for<16>([&](auto Row) { csum += landed(cs[decltype(Row)::value]); });
                         }
                         pa += 2 * kStepA;
                         pb += 2 * kStepB;
                     });
                step(a1v, b1v,
                     [&]() { a0v.template issue<0>(pa); b0v.template issue<0>(pb); },
                     [&]() { if (2 * it + 1 < NPA) piece_a(cnext, buf2, 2 * it + 1); },
                     [&]() { if (colsum_block && it + 1 < R / 16) cs_issue(it + 1); });
            }
#pragma unroll 1
            for (int it = 0; it < kSteps / 4; ++it) {
                const bool last = it == kSteps / 4 - 1;
                step(a0v, b0v,
                     [&]() { a1v.template issue<kStepA>(pa); b1v.template issue<kStepB>(pb); },
                     [&]() { if (2 * it < NPB) piece_b(cnext, buf2, 2 * it); },
                     [&]() {
                         // the pair after next; past the last pair the read is repeated on the current rows (never used):
                         // one loop shape for all iterations keeps the accumulators where they are
                         pa = last ? pa : pa + 2 * kStepA;
                         pb = last ? pb : pb + 2 * kStepB;
                     });
                step(a1v, b1v,
                     [&]() { a0v.template issue<0>(pa); b0v.template issue<0>(pb); },
                     [&]() { if (2 * it + 1 < NPB) piece_b(cnext, buf2, 2 * it + 1); },
                     [&]() {});
            }
        } else {
            // Two MFMAs per point pair (the 128 x 64 and 64 x 128 shapes): a pair is too short to hide anything behind, so a step
            // is TWO pairs -- four MFMAs, the reads of the next two pairs behind the first two of them, the piece behind the third,
            // pointer / column-sum work behind the fourth -- on four register sets.
            static_assert(M == 2 && kSteps % 8 == 0, "the two-pair schedule");
            LdsVec<NTW> a2v, a3v;
            LdsVec<KTW> b2v, b3v;
            a1v.template issue<kStepA>(pa);
            b1v.template issue<kStepB>(pb);
            auto quad = [&](LdsVec<NTW>& c0a, LdsVec<KTW>& c0b, LdsVec<NTW>& c1a, LdsVec<KTW>& c1b, LdsVec<NTW>& n0a, LdsVec<KTW>& n0b,
                            LdsVec<NTW>& n1a, LdsVec<KTW>& n1b, bool last, auto&& side_c, auto&& side_d) {
                lds_retire<0>(c0a, c0b);
                lds_retire<0>(c1a, c1b);
                // the two pairs after these; past the chunk's last pair the reads are repeated on the current rows (never used)
                const uint32_t na = last ? pa : pa + 2 * kStepA, nb = last ? pb : pb + 2 * kStepB;
                auto mf = [&](LdsVec<NTW>& ca, LdsVec<KTW>& cb, auto M_) {
                    constexpr int m = decltype(M_)::value, x = m / KTW, y = m % KTW;
                    acc[x][y] = mfma32(ca.get(x), cb.get(y), acc[x][y]);
                    __builtin_amdgcn_sched_barrier(0);
                };
                mf(c0a, c0b, ic<0>{});
                n0a.template issue<0>(na);
                n0b.template issue<0>(nb);
                __builtin_amdgcn_sched_barrier(0);
                mf(c0a, c0b, ic<1>{});
                n1a.template issue<kStepA>(na);
                n1b.template issue<kStepB>(nb);
                __builtin_amdgcn_sched_barrier(0);
                mf(c1a, c1b, ic<0>{});
                side_c();
                __builtin_amdgcn_sched_barrier(0);
                mf(c1a, c1b, ic<1>{});
                side_d();
                pa = na;
                pb = nb;
                __builtin_amdgcn_sched_barrier(0);
            };
#pragma unroll 1
            for (int it = 0; it < kSteps / 8; ++it) {
                quad(a0v, b0v, a1v, b1v, a2v, b2v, a3v, b3v, false,
                     [&]() { if (2 * it < NPA) piece_a(cnext, buf2, 2 * it); },
                     [&]() {
                         if (colsum_block && it < R / 16) {   // batch `it` of the column reads is older than these operand reads: retired with them
                             static_for<16>([&](auto Row) { csum += landed(cs[decltype(Row)::value]); });
                         }
                     });
                quad(a2v, b2v, a3v, b3v, a0v, b0v, a1v, b1v, false,
                     [&]() { if (2 * it + 1 < NPA) piece_a(cnext, buf2, 2 * it + 1); },
                     [&]() { if (colsum_block && it + 1 < R / 16) cs_issue(it + 1); });
            }
#pragma unroll 1
            for (int it = 0; it < kSteps / 8; ++it) {
                quad(a0v, b0v, a1v, b1v, a2v, b2v, a3v, b3v, false,
                     [&]() { if (2 * it < NPB) piece_b(cnext, buf2, 2 * it); }, [&]() {});
                quad(a2v, b2v, a3v, b3v, a0v, b0v, a1v, b1v, it == kSteps / 8 - 1,
                     [&]() { if (2 * it + 1 < NPB) piece_b(cnext, buf2, 2 * it + 1); }, [&]() {});
            }
            lds_retire<0>(a1v, b1v);
        }
        lds_retire<0>(a0v, b0v);   // drain the repeated read before these registers are reused
        buf = buf + 1 == NB ? 0 : buf + 1;
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // the clamped re-reads of the last chunk: nothing may land in LDS after this workgroup has left
    if (do_colsum) g.cpart[(long)split * g.N + n0 + tid] = csum;
    // this lane holds, for tile (x, y) register r: output (n0 + NTW (32 wr + d_row(r, hh)) + x, k0 + KTW (32 wc + i) + y):
    // the KTW values of one (x, r) are contiguous in a row of the partial block
    float* out = g.part + (long)split * g.N * g.K;
#pragma unroll
    for (int x = 0; x < NTW; ++x)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int n = n0 + NTW * (32 * wr + d_row(r, hh)) + x;
            float* dst = out + (long)n * g.K + k0 + KTW * (32 * wc + i);
            if constexpr (KTW == 4) {
                *reinterpret_cast<f32x4*>(dst) = f32x4{acc[x][0][r], acc[x][1][r], acc[x][2][r], acc[x][3][r]};
            } else {
#pragma unroll
                for (int y = 0; y < KTW; ++y) dst[y] = acc[x][y][r];
            }
        }
}

// ---------------------------------------------------------------------------
// The 256 x 256 dW GEMMs on the bf16 matrix pipe: every fp32 operand is the exact sum of three bf16 pieces
// (x = p1 + p2 + p3, each the round-to-nearest bf16 of what the pieces before it left: 3 x 8 significand bits
// and bf16 has fp32's exponent range, so nothing is scaled and nothing can overflow that fp32 holds), and a
// product keeps the six piece products down to 2^-16 of it,
//      a.b ~ a1 b1 + a1 b2 + a2 b1 + a2 b2 + a1 b3 + a3 b1      (dropped: a2 b3 + a3 b2 + a3 b3 <= 2^-23 |a b|),
// accumulated in fp32 by v_mfma_f32_32x32x16_bf16: the rounding of an fp32 fma chain (2^-24 per step), at
// 16 / 6 of the fp32 MFMA rate.  A block owns the whole 256 x 256 output of one split of the points.
//
// Data path per 16-point chunk: thread t loads column t of the delta tile and of the activation tile (16 dwords
// each, a row of the tile per wave instruction), splits them and stores the pieces FRAGMENT-READY in LDS --
// [matrix][32-channel tile][piece][lane (i, hh)][8 bf16 = points 8 hh .. 8 hh + 7 of channel i]: the thread's own
// 16 bytes per piece and lane half, conflict free -- while the chunk before is multiplied; the registers then take
// the chunk after next straight away, so a load has a whole chunk to land.  Two LDS buffers of 48 KiB, one
// counted wait + raw barrier per chunk.  The bias gradient (column sums of delta) is added up by the thread
// that holds the column anyway.
// ---------------------------------------------------------------------------
typedef unsigned tn_u32x4 __attribute__((ext_vector_type(4)));
typedef int tn_i32x4 __attribute__((ext_vector_type(4)));
// x6::split3 with the pieces as the words that go to LDS.  (No piece may be an MFMA operand directly -- x6::cvt_pk_bf16 -- and
// none is: each goes to LDS (`store`) and comes back through a fragment read; tools/audit_asm_loads.py check 4 enforces that.)
__device__ __forceinline__ void split3(float x0, float x1, unsigned& p1, unsigned& p2, unsigned& p3) {
    float w1, w2, w3;
    x6::split3(x0, x1, w1, w2, w3);
    p1 = __float_as_uint(w1), p2 = __float_as_uint(w2), p3 = __float_as_uint(w3);
}
constexpr int kX6BufBytes = 2 * 8 * 3 * kFragBytes;   // (delta, acts) x 8 tiles x 3 pieces x 1 KiB
constexpr int kX6Lds = 2 * kX6BufBytes;

struct X6Frag {
    f32x4 v;
    template <int OFF>
    __device__ __forceinline__ void issue(uint32_t addr) { asm volatile("ds_read_b128 %0, %1 offset:%2" : "=v"(v) : "v"(addr), "n"(OFF) : "memory"); }
};
// at most N of this wave's LDS operations are still outstanding => the three fragments named are valid
template <int N>
__device__ __forceinline__ void x6_retire(X6Frag (&f)[3]) {
    static_assert(N <= 15, "lgkmcnt is a 4-bit field");
    asm volatile("s_waitcnt lgkmcnt(%3)" : "+v"(f[0].v), "+v"(f[1].v), "+v"(f[2].v) : "n"(N) : "memory");
}

// One 256 x 256 product (one split of the points) of the batch below.
__device__ __forceinline__ void gemm_tn_x6_item(const TNArgs& g, const int split, char* x6_smem) {
    const int tid = threadIdx.x, lane = tid & 63;
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int i = lane & 31, hh = lane >> 5;
    const int wr = w >> 1, wc = w & 1;
    f32x16 acc[4][4];
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int b = 0; b < 4; ++b)
            for (int r = 0; r < 16; ++r) acc[a][b][r] = 0.f;

    const long c_begin = (long)split * g.chunks_per_split;
    long c_end = c_begin + g.chunks_per_split;
    const long c_total = g.P / kTnRows;
    if (c_end > c_total) c_end = c_total;
    const int n_chunks = (int)(c_end - c_begin);          // >= 1 (DwPass::product sizes the splits so)
    // Raw buffer descriptors based at this split's first row (32-bit offsets span one split).  The loads are inline asm
    // with the destination tied to the register that held the same row of the chunk before ("+v"): as a builtin the
    // reload got a fresh register and a copy at the loop end -- behind a wait for the load, a chunk early.  vmcnt is
    // therefore counted by hand: loads are issued in ONE order (delta rows 0..15, activation rows 0..15) everywhere,
    // so when pair j is split, exactly 30 loads are younger than its second row.
    // (With cache-hot reloads -- a timing-only build, profiles/r04_ab_x6_same_rows.log -- the kernel is 8 % faster; a second register set per matrix -- two
    // chunks in flight, vmcnt(62) -- was built and measured in round 4: no gain, so it is not the prefetch depth.  profiles/HISTORY.md)
    auto make_rsrc = [](const float* ptr) {
        const uint64_t a64 = (uint64_t)(uintptr_t)ptr;
        return tn_i32x4{(int)(uint32_t)a64, (int)((uint32_t)(a64 >> 32) & 0xffffu), (int)0xfffffffcu, 0x00020000};
    };
    const tn_i32x4 rsrcA = make_rsrc(g.A + c_begin * kTnRows * (long)g.lda);
    const tn_i32x4 rsrcB = make_rsrc(g.B + c_begin * kTnRows * (long)g.ldb);
    const int voff = tid * 4;
    const int voffB = g.b_split ? (tid < 128 ? g.b_off0 : g.b_off1) + (tid & 127) * 4 : voff;
    const int rowA = g.lda * 4, rowB = g.ldb * 4;
    float ra[kTnRows], rb[kTnRows];
#pragma unroll
    for (int p = 0; p < kTnRows; ++p) ra[p] = rb[p] = 0.f;
    auto load_row_at = [&](float& dst, const tn_i32x4& rsrc, int soff, int vo) {
        asm volatile("buffer_load_dword %0, %1, %2, %3 offen" : "+v"(dst) : "v"(vo), "s"(rsrc), "s"(soff) : "memory");
    };
    auto load_row = [&](float& dst, const tn_i32x4& rsrc, int soff) { load_row_at(dst, rsrc, soff, voff); };
    auto load_chunk = [&](int rc) {   // chunk rc of this split, clamped to its last one (re-read, never used)
        const int base = (rc < n_chunks ? rc : n_chunks - 1) * kTnRows;
#pragma unroll
        for (int p = 0; p < kTnRows; ++p) load_row(ra[p], rsrcA, (base + p) * rowA);
#pragma unroll
        for (int p = 0; p < kTnRows; ++p) load_row_at(rb[p], rsrcB, (base + p) * rowB, voffB);
    };
    // this thread's slot: tile tid / 32, lane (tid % 32, hh) -> hh-th half of the fragment
    char* const my_slot = x6_smem + (tid >> 5) * (3 * kFragBytes) + (tid & 31) * 16;
    auto split_store = [&](int buf, int X, const float (&r)[kTnRows]) {
        unsigned pw[3][8];
#pragma unroll
        for (int j = 0; j < 8; ++j) split3(r[2 * j], r[2 * j + 1], pw[0][j], pw[1][j], pw[2][j]);
        char* dst = my_slot + buf * kX6BufBytes + X * (8 * 3 * kFragBytes);
#pragma unroll
        for (int q = 0; q < 3; ++q)
#pragma unroll
            for (int h2 = 0; h2 < 2; ++h2)
                *reinterpret_cast<tn_u32x4*>(dst + q * kFragBytes + h2 * 512) =
                    tn_u32x4{pw[q][4 * h2], pw[q][4 * h2 + 1], pw[q][4 * h2 + 2], pw[q][4 * h2 + 3]};
    };
    const bool do_colsum = g.cpart != nullptr;
    float csum = 0.0f, csum1 = 0.0f;
    auto colsum = [&]() {   // chunk 0 (the loop adds the others as it splits them)
        float s0 = (ra[0] + ra[1]) + (ra[2] + ra[3]), s1 = (ra[4] + ra[5]) + (ra[6] + ra[7]);
        float s2 = (ra[8] + ra[9]) + (ra[10] + ra[11]), s3 = (ra[12] + ra[13]) + (ra[14] + ra[15]);
        csum += (s0 + s1) + (s2 + s3);
    };
    const uint32_t smem0 = (uint32_t)(uintptr_t)(__attribute__((address_space(3))) char*)x6_smem;
    const uint32_t a_base = smem0 + (4 * wr) * (3 * kFragBytes) + lane * 16;
    const uint32_t b_base = smem0 + (8 + 4 * wc) * (3 * kFragBytes) + lane * 16;

    load_chunk(0);
#pragma unroll
    for (int p = 0; p < kTnRows; ++p) asm volatile("s_waitcnt vmcnt(0)" : "+v"(ra[p]), "+v"(rb[p])::"memory");
    colsum();
    split_store(0, 0, ra);
    split_store(0, 1, rb);
    load_chunk(1);
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    asm volatile("" ::: "memory");

    // The fragments of a chunk's FIRST tile row (fa[0], fb[0], fb[1]: nine reads) are issued one chunk EARLY: the chunk barrier
    // sits behind MFMA 59 of the 72 of rows 1..3 -- by then this wave's pieces of the next chunk are stored (slices end at MFMA
    // 51) and fa[0] / fb[0] / fb[1] have had their last use -- so the next chunk's first reads run under the last twelve MFMAs
    // instead of behind a barrier with nothing to overlap (profiles/r04_ab_x6_early_barrier.log).
    X6Frag fa[4][3], fb[4][3];
    auto issue_first_row = [&](uint32_t pa, uint32_t pb) {
        static_for<3>([&](auto Q) { fa[0][decltype(Q)::value].template issue<decltype(Q)::value * kFragBytes>(pa); });
        static_for<2>([&](auto Y) {
            static_for<3>([&](auto Q) {
                fb[decltype(Y)::value][decltype(Q)::value].template issue<(decltype(Y)::value * 3 + decltype(Q)::value) * kFragBytes>(pb);
            });
        });
    };
    issue_first_row(a_base, b_base);
#pragma unroll 1
    for (int rc = 0; rc < n_chunks; ++rc) {
        const int buf = rc & 1;
        const uint32_t pa = a_base + buf * kX6BufBytes, pb = b_base + buf * kX6BufBytes;
        // issue order = consumption order: row 0 (nine of its reads are already in flight), then the other delta tiles
        static_for<2>([&](auto Y) {
            static_for<3>([&](auto Q) {
                fb[decltype(Y)::value + 2][decltype(Q)::value].template issue<((decltype(Y)::value + 2) * 3 + decltype(Q)::value) * kFragBytes>(pb);
            });
        });
        static_for<3>([&](auto X) {
            static_for<3>([&](auto Q) {
                fa[decltype(X)::value + 1][decltype(Q)::value].template issue<((decltype(X)::value + 1) * 3 + decltype(Q)::value) * kFragBytes>(pa);
            });
        });
        auto mm2 = [&](int x, int y0, int y1) {   // two tile pairs, interleaved: six piece products each
#define X6_TERM(QA, QB)                                                   \
    acc[x][y0] = x6::mfma_bf(fa[x][QA].v, fb[y0][QB].v, acc[x][y0]);        \
    acc[x][y1] = x6::mfma_bf(fa[x][QA].v, fb[y1][QB].v, acc[x][y1]);
            X6_TERM(0, 0) X6_TERM(0, 1) X6_TERM(1, 0) X6_TERM(1, 1) X6_TERM(0, 2) X6_TERM(2, 0)
#undef X6_TERM
        };
        // row 0: 24 reads are outstanding; fa[0], fb[0], fb[1] are the oldest nine
        x6_retire<15>(fa[0]);
        x6_retire<15>(fb[0]);
        x6_retire<15>(fb[1]);
        mm2(0, 0, 1);
        x6_retire<9>(fb[2]);
        x6_retire<9>(fb[3]);
        mm2(0, 2, 3);
        x6_retire<0>(fa[1]);
        x6_retire<0>(fa[2]);
        x6_retire<0>(fa[3]);
        // Rows 1..3: 72 MFMAs, each followed by one SLICE of the side work (the next chunk's split + store, the reloads
        // with the chunk after it) and a scheduling fence: at most ~6 vector instructions, two loads or one store behind
        // an MFMA that occupies the pipe for 32 cycles.  (Left alone, hipcc issues 40 MFMAs back to back and then 50
        // vector and memory instructions in a row, during which the matrix pipe runs dry: 57 % busy.)
        const unsigned live_mask = rc + 1 < n_chunks ? 0xffffffffu : 0u;   // the clamped re-read of the last chunk does not count
        const int nbase = (rc + 2 < n_chunks ? rc + 2 : n_chunks - 1) * kTnRows;   // chunk rc + 2, clamped (re-read, never used)
        char* const dst = my_slot + (buf ^ 1) * kX6BufBytes;
        unsigned pw[2][3][8];
        float t0 = 0.f, t1 = 0.f;
        auto slice = [&](auto X_, auto S_) {
            constexpr int X = decltype(X_)::value, sl = decltype(S_)::value;
            float (&r)[kTnRows] = *(X ? &rb : &ra);
            auto store = [&](auto Q_, auto H_) {
                constexpr int q = decltype(Q_)::value, h2 = decltype(H_)::value;
                *reinterpret_cast<tn_u32x4*>(dst + X * (8 * 3 * kFragBytes) + q * kFragBytes + h2 * 512) =
                    tn_u32x4{pw[X][q][4 * h2], pw[X][q][4 * h2 + 1], pw[X][q][4 * h2 + 2], pw[X][q][4 * h2 + 3]};
            };
            if constexpr (sl < 24) {
                constexpr int j = sl / 3, ph = sl % 3;
                if constexpr (ph == 0) {
                    // rows 2 j, 2 j + 1 of the chunk being split have landed: 30 younger loads may still be in flight
                    asm volatile("s_waitcnt vmcnt(30)" : "+v"(r[2 * j]), "+v"(r[2 * j + 1])::"memory");
                    const unsigned p1 = x6::cvt_pk_bf16(r[2 * j], r[2 * j + 1]);
                    pw[X][0][j] = p1;
                    t0 = r[2 * j] - __uint_as_float(p1 << 16);
                    t1 = r[2 * j + 1] - __uint_as_float(p1 & 0xffff0000u);
                    if constexpr (X == 0) {   // (masked, not multiplied: packed-fp32 forms would tie the reload registers to aligned pairs)
                        csum += __uint_as_float(__float_as_uint(r[2 * j]) & live_mask);
                        csum1 += __uint_as_float(__float_as_uint(r[2 * j + 1]) & live_mask);
                        // pinned here: hipcc otherwise keeps the 16 values for one batch of adds at the end, i.e. copies every
                        // row register before its reload (and copies in-flight registers back at the loop end)
                        asm volatile("" : "+v"(csum), "+v"(csum1));
                    }
                } else if constexpr (ph == 1) {
                    const unsigned p2 = x6::cvt_pk_bf16(t0, t1);
                    pw[X][1][j] = p2;
                    t0 = t0 - __uint_as_float(p2 << 16);
                    t1 = t1 - __uint_as_float(p2 & 0xffff0000u);
                    pw[X][2][j] = x6::cvt_pk_bf16(t0, t1);
                } else {
                    load_row_at(r[2 * j], X ? rsrcB : rsrcA, (nbase + 2 * j) * (X ? rowB : rowA), X ? voffB : voff);
                    load_row_at(r[2 * j + 1], X ? rsrcB : rsrcA, (nbase + 2 * j + 1) * (X ? rowB : rowA), X ? voffB : voff);
                    if constexpr (j >= 3 && j < 6) store(ic<j - 3>{}, ic<0>{});
                    if constexpr (j == 7) store(ic<0>{}, ic<1>{});
                }
            } else if constexpr (sl == 24) {
                store(ic<1>{}, ic<1>{});
            } else if constexpr (sl == 25) {
                store(ic<2>{}, ic<1>{});
            }
        };
        __builtin_amdgcn_sched_barrier(0);
        static_for<72>([&](auto K_) {
            constexpr int k = decltype(K_)::value;
            constexpr int x = 1 + k / 24, kk = k % 24, y = 2 * (kk / 12) + (kk % 2), t = (kk % 12) / 2;
            constexpr int qa = t == 2 || t == 3 ? 1 : (t == 5 ? 2 : 0);   // a1 b1, a1 b2, a2 b1, a2 b2, a1 b3, a3 b1
            constexpr int qb = t == 1 || t == 3 ? 1 : (t == 4 ? 2 : 0);
            acc[x][y] = x6::mfma_bf(fa[x][qa].v, fb[y][qb].v, acc[x][y]);
            constexpr int kX1 = 26;     // where the activation matrix's slices start (each matrix has 26)
            if constexpr (k < kX1) slice(ic<0>{}, ic<k>{});
            else slice(ic<1>{}, ic<k - kX1>{});
            if constexpr (k == 59) {
                // everyone's pieces of chunk rc + 1 are in LDS; everyone has read chunk rc's (all 24 fragment reads were retired
                // before row 1): the chunk barrier, twelve MFMAs early, and behind it the first row of the next chunk
                asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
                __builtin_amdgcn_s_barrier();
                asm volatile("" ::: "memory");
                issue_first_row(a_base + (buf ^ 1) * kX6BufBytes, b_base + (buf ^ 1) * kX6BufBytes);
            }
            __builtin_amdgcn_sched_barrier(0);
        });
    }
    // the first-row reads issued behind the last chunk's barrier (of a chunk that does not exist): retired, never used
    x6_retire<0>(fa[0]);
    x6_retire<0>(fb[0]);
    x6_retire<0>(fb[1]);
    // the clamped re-reads of the last chunk are still in flight into ra / rb: retired here, so that the next item of a batch
    // starts on registers nothing is about to write (the stores below then drain under that item's first loads)
#pragma unroll
    for (int p = 0; p < kTnRows; ++p) asm volatile("s_waitcnt vmcnt(0)" : "+v"(ra[p]), "+v"(rb[p])::"memory");
    if (do_colsum) g.cpart[(long)split * g.N + tid] = csum + csum1;
    // lane (i, hh), tile (x, y), register r: output (32 (4 wr + x) + d_row(r, hh), 32 (4 wc + y) + i)
    float* out = g.part + (long)split * g.N * g.K;
#pragma unroll
    for (int x = 0; x < 4; ++x)
#pragma unroll
        for (int y = 0; y < 4; ++y)
#pragma unroll
            for (int r = 0; r < 16; ++r)
                out[(long)(32 * (4 * wr + x) + d_row(r, hh)) * g.K + 32 * (4 * wc + y) + i] = acc[x][y][r];
}
// The 256 x 256 weight-gradient products of a pass as ONE launch, ONE PRODUCT PER WORKGROUP: workgroup z works on item
// z / splits over split z % splits of the points, with splits = 2 #CUs / #items (56 for the nine products of a pass on 256 CUs).
// Round 3 walked all items in every workgroup (256 splits each): 9 x 256 partial blocks of 256 KB per pass -- 590 MB written
// and read back by the reduction, whatever the number of points (17 % of the coarse pass's traffic).  Now a workgroup keeps
// its accumulators over 1 / 56 of the points and writes ONE block: 131 MB per pass, and the reduction reads less than a quarter.
__global__ __launch_bounds__(256) void gemm_tn_x6_kernel(TNBatch b) {
    extern __shared__ __attribute__((aligned(16))) char x6_smem[];
    const int item = __builtin_amdgcn_readfirstlane((int)blockIdx.z / b.splits);
    const int split = __builtin_amdgcn_readfirstlane((int)blockIdx.z - item * b.splits);
    gemm_tn_x6_item(b.it[item], split, x6_smem);
}

// out[n*ldo + k] = sum_s part[s][n][k],  n < rows, k < cols  (rows/cols may be smaller than N/K: padding dropped)
// 64 outputs x 4 split lanes per block: lane q adds splits q, q+4, ... in fp64, the four lanes are
// then added in a fixed order (deterministic), so 4x as many loads are in flight per output.
// All partial-slab reductions of a pass in ONE launch (they were 27 launches of a few microseconds each per
// pass, each waiting for the one before it).  Block b works on the item whose block range holds b.
__global__ __launch_bounds__(256) void reduce_batch_kernel(ReduceBatch b) {
    __shared__ double red[4][64];
    int i = 0;
    while (i + 1 < b.n && (int)blockIdx.x >= b.it[i].block_end) ++i;   // block-uniform
    const ReduceItem& t = b.it[i];
    const int block0 = i ? b.it[i - 1].block_end : 0;
    const int o = threadIdx.x & 63, q = threadIdx.x >> 6;
    const int idx = ((int)blockIdx.x - block0) * 64 + o;
    const bool live = idx < t.rows * t.cols;
    const int n = live ? idx / t.cols : 0, k = live ? idx % t.cols : 0;
    double s = 0.0;
    if (live) {
        const float* src = t.part + (long)n * t.K + k;
        const long stride = (long)t.N * t.K;
#pragma unroll 8
        for (int sp = q; sp < t.splits; sp += 4) s += (double)src[sp * stride];
    }
    red[q][o] = s;
    __syncthreads();
    if (q == 0 && live) t.out[(long)n * t.ldo + k] = (float)(((red[0][o] + red[1][o]) + red[2][o]) + red[3][o]);
}

// ---- host: the products of a pass (DwPass, dw_gemm.h) ----
template <int NTW, int KTW, int NB, int R = kTnRows>
static int launch_tn(const TNArgs& g, int splits, hipStream_t s) {
    constexpr size_t lds = (size_t)NB * R * (size_t)(64 * NTW + 64 * KTW) * 4;
    static_assert(lds <= 160 * 1024, "the chunk ring must fit a CU's LDS");
    static LaunchSetup setup;
    int num_cu = 0;
    if (int e = setup.get([]() -> int {
            IDN_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(&gemm_tn_kernel<NTW, KTW, NB, R>),
                                              hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
            return IDN_OK;
        }, &num_cu))
        return e;
    hipLaunchKernelGGL((gemm_tn_kernel<NTW, KTW, NB, R>), dim3(g.N / (64 * NTW), g.K / (64 * KTW), splits), dim3(256), lds, s, g);
    IDN_HIP_CHECK(hipGetLastError());
    return IDN_OK;
}
// One row per instantiation: the N x K outputs it computes (every one a single block column: the grid is 1 x 1 x splits), the
// points per chunk, the most splits it runs and its launcher (null: queued for the pass's one gemm_tn_x6_kernel launch, with
// 2 #CUs / #items splits).  The narrow rows -- 256 x 64, 128 x 64, 64 x 128 -- take the larger chunks (gemm_tn_kernel).
struct DwShape { int N, K, rows_per_chunk, max_splits; int (*launch)(const TNArgs&, int, hipStream_t); };
constexpr DwShape kX6Shape = {256, 256, kTnRows, kMaxSplits, nullptr};
constexpr DwShape kF32Shapes[] = {
    {256, 256, kTnRows, kMaxSplits, &launch_tn<4, 4, kTnBufs>},
    {256, 64, kTnRows4x1, kTnNarrowSplits, &launch_tn<4, 1, kTnNarrowBufs, kTnRows4x1>},      // pts_linears.0, the encoding columns of pts_linears.5
    {128, 256, kTnRows, kMaxSplits, &launch_tn<2, 4, kTnBufs>},                               // views_linears.0: its 128 units x the 256 trunk channels
    {128, 64, kTnRowsThin, kTnNarrowSplits, &launch_tn<2, 1, kTnNarrowBufs, kTnRowsThin>},    //                  ... x the direction encoding
    {128, 128, kTnRows, kMaxSplits, &launch_tn<2, 2, kTnBufs>},
    {64, 128, kTnRowsThin, kTnNarrowSplits, &launch_tn<1, 2, kTnNarrowBufs, kTnRowsThin>},    // rgb_linear
};
static_assert(kTnNarrowSplits <= kMaxSplits, "the pools hold kMaxSplits splits of every product of a pass (dw_gemm.h)");

static int x6_setup(int* cus) {   // gemm_tn_x6_kernel's LDS opt-in and the CUs it shares out, once per device
    static LaunchSetup st;
    return st.get([]() -> int {
        IDN_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(&gemm_tn_x6_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, kX6Lds));
        return IDN_OK;
    }, cus);
}

int DwPass::product(const float* A, int lda, int N, const float* B, int ldb, int K, bool want_colsum, DwProduct* h, const float* B2) {
    const DwShape* sh = nullptr;
    if (N == 256 && K == 256 && pipe == kPipeX6) sh = &kX6Shape;
    else
        for (const DwShape& t : kF32Shapes)
            if (t.N == N && t.K == K) sh = &t;
    if (!sh) return fail(IDN_EUNSUPPORTED, "gemm_tn: no instantiation for %d x %d", N, K);
    const bool queued = sh->launch == nullptr;
    if (B2 && !queued) return fail(IDN_EINVAL, "gemm_tn: a split B needs the 256 x 256 bf16-piece kernel");
    if (P % sh->rows_per_chunk) return fail(IDN_EINVAL, "gemm_tn: %lld rows are not a multiple of the %d-row chunk", (long long)P, sh->rows_per_chunk);
    const long chunks = P / sh->rows_per_chunk;
    int splits = sh->max_splits;
    if (queued) {   // one product per workgroup: the CUs are divided among the pass's products
        if (x6.n >= x6_items || x6.n >= kMaxTnBatch) return fail(IDN_EINVAL, "gemm_tn: more 256 x 256 products than the pass declared (%d)", x6_items);
        int cus = 0;
        if (int e = x6_setup(&cus)) return e;
        // two rounds of workgroups per CU: the tail is still balanced (2 x 28 x 9 = 504 workgroups on 256 CUs), the fp32 accumulators
        // run over 1 / 56 of the points (10 500 of the fine pass's 589 824) and the partial blocks are 131 MB per pass
        splits = 2 * cus / x6_items;
        if (splits > kMaxSplits) splits = kMaxSplits;
    }
    if (splits > chunks) splits = (int)chunks;
    if (splits < 1) splits = 1;
    const int cps = (int)((chunks + splits - 1) / splits);
    splits = (int)((chunks + cps - 1) / cps);
    const size_t part_floats = (size_t)splits * N * K, cpart_floats = want_colsum ? (size_t)splits * N : 0;
    if (part_floats > part_left || cpart_floats > cpart_left)
        return fail(IDN_EWORKSPACE, "gemm_tn: the partial blocks of %d x %d in %d splits do not fit the pool", N, K, splits);
    TNArgs g{A, lda, B, ldb, part_next, N, K, (long)P, cps, want_colsum ? cpart_next : nullptr, 0, 0, 0};
    if (B2) {   // byte offsets from the lower of the two addresses (buffer offsets are unsigned)
        const float* base = B < B2 ? B : B2;
        const int64_t o0 = (int64_t)(B - base) * 4, o1 = (int64_t)(B2 - base) * 4;
        if (o0 >= (int64_t)1 << 31 || o1 >= (int64_t)1 << 31) return fail(IDN_EUNSUPPORTED, "gemm_tn: split B matrices more than 2 GiB apart");
        g.B = base, g.b_split = 1;
        g.b_off0 = (int)o0, g.b_off1 = (int)o1;
    }
    if (queued) {   // launched with the pass's other 256 x 256 products (finish): same rows, same item count, so the same splits
        x6.splits = splits;
        x6.it[x6.n++] = g;
    } else {
        ProfScope prof(s, P, IDN_PROF_DW_GEMM);
        if (int e = sh->launch(g, splits, s)) return e;
    }
    *h = DwProduct{g.part, g.cpart, splits, N, K, cps};
    part_next += part_floats, part_left -= part_floats;
    cpart_next += cpart_floats, cpart_left -= cpart_floats;
    return IDN_OK;
}

int DwPass::take(const DwProduct& h, int row0, int col0, int rows, int cols, float* out, int ldo) {
    if (red.n >= kMaxReduceItems) return fail(IDN_EUNSUPPORTED, "reduce queue full");
    red_blocks += (rows * cols + 63) / 64;
    red.it[red.n++] = ReduceItem{h.part + (size_t)row0 * h.K + col0, out, h.splits, h.N, h.K, ldo, rows, cols, red_blocks};
    return IDN_OK;
}
int DwPass::take_colsum(const DwProduct& h, int col0, int cols, float* out) {   // the column sums are a 1 x N block per split
    if (!h.cpart) return fail(IDN_EINVAL, "gemm_tn: the product kept no column sums");
    return take(DwProduct{h.cpart, nullptr, h.splits, 1, h.N, h.chunks_per_split}, 0, col0, 1, cols, out, cols);
}

int DwPass::finish() {   // once: the queues are not reset
    if (x6.n) {
        ProfScope prof(s, P * x6.n, IDN_PROF_DW_GEMM_X6);
        hipLaunchKernelGGL(gemm_tn_x6_kernel, dim3(1, 1, x6.splits * x6.n), dim3(256), kX6Lds, s, x6);
    }
    IDN_HIP_CHECK(hipGetLastError());
    if (red.n) hipLaunchKernelGGL(reduce_batch_kernel, dim3(red_blocks), dim3(256), 0, s, red);
    IDN_HIP_CHECK(hipGetLastError());
    return IDN_OK;
}

size_t dw_gemm_workspace_bytes() { return al256((size_t)kMaxSplits * 65536 * 4) + al256((size_t)kColsumBlocks * 256 * 4); }
int launch_dw_gemm(const float* delta, int ld_delta, const float* acts, int ld_acts, int64_t rows, float* dW, float* db, int pipe,
                   void* ws, size_t ws_bytes, hipStream_t s) {
    if (rows <= 0 || rows % 128) return fail(IDN_EINVAL, "dw_gemm: rows %lld is not a positive multiple of 128", (long long)rows);
    if (ld_delta < 256 || ld_acts < 256) return fail(IDN_EINVAL, "dw_gemm: row pitch < 256");
    // IDN_DW_PIPE_BF16X6_PASS: the split count a pass runs its nine products with
    const int x6_items = pipe == IDN_DW_PIPE_BF16X6_PASS ? kX6ItemsPerPass : 1;
    if (pipe == IDN_DW_PIPE_BF16X6_PASS) pipe = IDN_DW_PIPE_BF16X6;
    if (pipe != IDN_DW_PIPE_BF16X6 && pipe != IDN_DW_PIPE_F32) return fail(IDN_EINVAL, "dw_gemm: pipe %d", pipe);
    if (!ws || ws_bytes < dw_gemm_workspace_bytes()) return fail(IDN_EWORKSPACE, "dw_gemm workspace %zu < %zu", ws_bytes, dw_gemm_workspace_bytes());
    float* part = reinterpret_cast<float*>(ws);
    float* cpart = reinterpret_cast<float*>(reinterpret_cast<char*>(ws) + al256((size_t)kMaxSplits * 65536 * 4));
    DwPass q(part, (size_t)kMaxSplits * 65536, cpart, (size_t)kColsumBlocks * 256, rows, pipe, x6_items, s);
    DwProduct h;
    if (int e = q.product(delta, ld_delta, 256, acts, ld_acts, 256, db != nullptr, &h)) return e;
    int e = db ? q.take_colsum(h, 0, 256, db) : IDN_OK;
    if (!e) e = q.take(h, 0, 0, 256, 256, dW, 256);
    return e ? e : q.finish();
}

// A list of products through ONE DwPass over pools of a pass's size (carve_bwd, train.hip), named as bwd_tail names them:
// product, its column-sum takes, its takes; finish.  Everything that can be refused without the device is refused in a first
// walk over the records, before DwPass::product touches HIP (it opts the x6 kernel into its LDS and launches the fp32 shapes
// as they are named).
size_t dw_products_workspace_bytes() { return al256(kPartPoolFloats * 4) + al256(kCpartPoolFloats * 4); }
int launch_dw_products(int64_t rows, int pipe, int x6_items, idn_dw_product* pr, int n, void* ws, size_t ws_bytes, hipStream_t s) {
    if (!pr) return fail(IDN_EINVAL, "dw_products: NULL pointer");
    if (n < 1 || n > IDN_DW_MAX_PRODUCTS) return fail(IDN_EINVAL, "dw_products: %d products outside [1, %d]", n, IDN_DW_MAX_PRODUCTS);
    if (pipe != kPipeX6 && pipe != kPipeF32) return fail(IDN_EINVAL, "dw_products: pipe %d", pipe);
    if (rows <= 0 || rows % 128) return fail(IDN_EINVAL, "dw_products: rows %lld is not a positive multiple of 128", (long long)rows);
    if (rows > (int64_t)1 << 24) return fail(IDN_EUNSUPPORTED, "dw_products: rows %lld exceed 2^24", (long long)rows);
    if (pipe == kPipeX6 && (x6_items < 1 || x6_items > kMaxTnBatch))
        return fail(IDN_EINVAL, "dw_products: x6_items %d outside [1, %d]", x6_items, kMaxTnBatch);
    int n_x6 = 0, n_red = 0;
    size_t part_per_split = 0, cpart_per_split = 0;
    for (int i = 0; i < n; ++i) {
        const idn_dw_product& t = pr[i];
        if (!t.delta || !t.acts) return fail(IDN_EINVAL, "dw_products: product %d: NULL pointer", i);
        const bool x6 = t.N == 256 && t.K == 256 && pipe == kPipeX6;
        bool known = x6;
        for (const DwShape& sh : kF32Shapes) known = known || (sh.N == t.N && sh.K == t.K);
        if (!known) return fail(IDN_EUNSUPPORTED, "dw_products: product %d: no instantiation for %d x %d", i, t.N, t.K);
        const int b_cols = t.acts2 ? 128 : t.K;   // a split B: two 128-column matrices
        if (t.ld_delta < t.N || t.ld_acts < b_cols) return fail(IDN_EINVAL, "dw_products: product %d: row pitch %d / %d < %d / %d", i, t.ld_delta, t.ld_acts, t.N, b_cols);
        // the fp32 kernels move 16-byte pieces of a row
        if (t.ld_delta % 4 || t.ld_acts % 4 || ((uintptr_t)t.delta | (uintptr_t)t.acts | (uintptr_t)t.acts2) % 16)
            return fail(IDN_EINVAL, "dw_products: product %d: operands are not 16-byte aligned row by row", i);
        if (t.acts2 && !x6) return fail(IDN_EINVAL, "dw_products: product %d: a split B needs the 256 x 256 bf16-piece kernel", i);
        if (t.acts2) {   // the kernel reaches both matrices from the lower address with 32-bit byte offsets (DwPass::product)
            const uintptr_t lo = (uintptr_t)(t.acts < t.acts2 ? t.acts : t.acts2), hi = (uintptr_t)(t.acts < t.acts2 ? t.acts2 : t.acts);
            if (hi - lo >= (uintptr_t)1 << 31) return fail(IDN_EUNSUPPORTED, "dw_products: product %d: split B matrices more than 2 GiB apart", i);
        }
        if (x6 && ++n_x6 > x6_items) return fail(IDN_EINVAL, "dw_products: more 256 x 256 products than x6_items (%d)", x6_items);
        if (t.n_takes < 0 || t.n_takes > IDN_DW_MAX_TAKES || t.n_colsum_takes < 0 || t.n_colsum_takes > IDN_DW_MAX_COLSUM_TAKES)
            return fail(IDN_EINVAL, "dw_products: product %d: %d takes / %d column-sum takes", i, t.n_takes, t.n_colsum_takes);
        if (t.n_colsum_takes && !t.want_colsum) return fail(IDN_EINVAL, "dw_products: product %d kept no column sums", i);
        if ((n_red += t.n_takes + t.n_colsum_takes) > kMaxReduceItems)
            return fail(IDN_EINVAL, "dw_products: more than %d takes in one pass", kMaxReduceItems);
        for (int j = 0; j < t.n_takes; ++j) {
            const idn_dw_take& k = t.takes[j];
            if (!k.out) return fail(IDN_EINVAL, "dw_products: product %d take %d: NULL pointer", i, j);
            if (k.row0 < 0 || k.col0 < 0 || k.rows < 1 || k.cols < 1 || k.row0 + k.rows > t.N || k.col0 + k.cols > t.K || k.ldo < k.cols)
                return fail(IDN_EINVAL, "dw_products: product %d take %d leaves the %d x %d block (or its pitch is short)", i, j, t.N, t.K);
        }
        for (int j = 0; j < t.n_colsum_takes; ++j) {
            const idn_dw_colsum_take& k = t.colsum_takes[j];
            if (!k.out) return fail(IDN_EINVAL, "dw_products: product %d column-sum take %d: NULL pointer", i, j);
            if (k.col0 < 0 || k.cols < 1 || k.col0 + k.cols > t.N)
                return fail(IDN_EINVAL, "dw_products: product %d column-sum take %d leaves the %d columns", i, j, t.N);
        }
        part_per_split += (size_t)t.N * t.K;
        cpart_per_split += t.want_colsum ? t.N : 0;
    }
    // no product runs more than kMaxSplits splits: the list fits the pools if one split of it does (as a pass's does, dw_gemm.h)
    if (part_per_split > kPartFloatsPerSplit || cpart_per_split * kMaxSplits > kCpartPoolFloats)
        return fail(IDN_EWORKSPACE, "dw_products: the list's partial blocks do not fit the pools of a pass");
    if (!ws || ws_bytes < dw_products_workspace_bytes())
        return fail(IDN_EWORKSPACE, "dw_products workspace %zu < %zu", ws_bytes, dw_products_workspace_bytes());
    float* part = reinterpret_cast<float*>(ws);
    float* cpart = reinterpret_cast<float*>(reinterpret_cast<char*>(ws) + al256(kPartPoolFloats * 4));
    DwPass q(part, kPartPoolFloats, cpart, kCpartPoolFloats, rows, pipe, x6_items, s);
    for (int i = 0; i < n; ++i) {
        idn_dw_product& t = pr[i];
        DwProduct h;
        if (int e = q.product(t.delta, t.ld_delta, t.N, t.acts, t.ld_acts, t.K, t.want_colsum != 0, &h, t.acts2)) return e;
        for (int j = 0; j < t.n_colsum_takes; ++j)
            if (int e = q.take_colsum(h, t.colsum_takes[j].col0, t.colsum_takes[j].cols, t.colsum_takes[j].out)) return e;
        for (int j = 0; j < t.n_takes; ++j) {
            const idn_dw_take& k = t.takes[j];
            if (int e = q.take(h, k.row0, k.col0, k.rows, k.cols, k.out, k.ldo)) return e;
        }
        t.splits = h.splits, t.chunks_per_split = h.chunks_per_split;
    }
    return q.finish();
}

}  // namespace idn
