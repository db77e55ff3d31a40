// Internal declarations shared by the HIP translation units of libidealnerf.so.
// gfx950 only.  See DESIGN.md for the data layout this header encodes.
#pragma once
#include <hip/hip_runtime.h>
#include <mutex>
#include <type_traits>
#include <stdint.h>
#include <stddef.h>
#include "../../include/idealnerf.h"

namespace idn {

// ---------------------------------------------------------------------------
// Packed weight stream (fp32 path).
//
// The per-point part of one FaceNeRF is a flat sequence of 1 KiB "fragments" in the
// exact order the kernel consumes them.  Fragment (layer, g, t) holds, for lane
// l = (i = l & 31, h = l >> 5), the four floats
//      W_layer[n = 32 t + i][k = 8 g + 4 h + j],  j = 0..3
// i.e. the A operands of four consecutive v_mfma_f32_32x32x2_f32 whose B operands
// are registers 4q..4q+3 (q = g & 3) of accumulator tile T = g >> 2 of the previous
// layer: an accumulator register r of tile T holds, in lane half h, output channel
// 32 T + (r & 3) + 8 (r >> 2) + 4 h = 8 g + 4 h + j.  Activations therefore never
// leave registers between layers.
//
// Within a layer, fragments are ordered tile-major (all k-groups of n-tile 0, then tile 1,
// ...), so output tiles finish one after the other and their ReLU / the next tile's bias load
// ride in the MFMA shadow of the neighbouring tile.  K sources are concatenated in
// k-groups of 8 channels (zero padded): PE(63 -> 8 groups), hidden (256 -> 32 groups),
// direction PE (27 -> 4 groups).  The conditioning columns are not in the stream; they
// are folded into the per-frame bias block (idealnerf_fold_conditioning).
// ---------------------------------------------------------------------------
// Encoding widths of a network (include/idealnerf.h: the params struct stores multires + 1, 0 = the default): the number
// of input columns that exist, 3 + 6 multires.  gamma_L is a prefix of gamma_10, the stream's K tiles are padded to 64 / 32
// columns whatever the width, and the packers zero every column the network does not have.
__host__ __device__ inline int pts_ch_of(const idn_facenerf_params& p) {
    return p.multires_plus1 ? 6 * p.multires_plus1 - 3 : IDN_PTS_CH;
}
__host__ __device__ inline int views_ch_of(const idn_facenerf_params& p) {
    return p.multires_views_plus1 ? 6 * p.multires_views_plus1 - 3 : IDN_VIEWS_CH;
}
// the two widths as the x-mode entries take them: 3 + 6 L with L in range
inline bool widths_ok(int pts_ch, int views_ch) {
    return pts_ch >= 3 && pts_ch <= IDN_PTS_CH && pts_ch % 6 == 3 && views_ch >= 3 && views_ch <= IDN_VIEWS_CH && views_ch % 6 == 3;
}

constexpr int kFragBytes = 1024;
constexpr int kFragFloats = 256;
// Ring geometry.  Measured on the bf16x3 kernel (512^2 frame): 2 x 64 KiB 4.12e8 samples/s,
// 4 x 32 KiB (prefetch three slices ahead, counted vmcnt) 3.98e8: the extra barriers cost more
// than the deeper prefetch buys; the stream's cost is its issue/bandwidth (timing-only build
// without it: 4.70e8), not its latency.
constexpr int kSliceFrags = 64;                 // one LDS ring slot = 64 KiB
constexpr int kRingSlots = 2;                   // slices are fetched kRingSlots-1 ahead of their use
constexpr int kRingFrags = kRingSlots * kSliceFrags;  // 128 KiB ring
constexpr int kSliceBytes = kSliceFrags * kFragBytes;

constexpr int kNumLayers = 12;  // pts0..7, views0(+alpha), views1, views2, rgb
// n-tiles (of 32 output channels) and k-groups (of 8 input channels) per layer
constexpr int kLayerNT[kNumLayers] = {8, 8, 8, 8, 8, 8, 8, 8, 5, 4, 4, 1};
constexpr int kLayerKG[kNumLayers] = {8, 32, 32, 32, 32, 40, 32, 32, 36, 16, 16, 16};

constexpr int layer_f0(int l) {
    int f = 0;
    for (int i = 0; i < l; ++i) f += kLayerNT[i] * kLayerKG[i];
    return f;
}
constexpr int kUsedFrags = layer_f0(kNumLayers);                                  // 2244
constexpr int kNumSlices =
    ((kUsedFrags + kSliceFrags - 1) / kSliceFrags + kRingSlots - 1) / kRingSlots * kRingSlots;  // 36
constexpr int kStreamFrags = kNumSlices * kSliceFrags;                            // 2304
static_assert(kUsedFrags == 2244, "layer table changed");
static_assert(kNumSlices % kRingSlots == 0, "slot of a slice must be static across passes");
static_assert(kRingFrags == 128, "FragReader addresses the ring as two 64-fragment halves");

// Plain-bf16 stream (IDN_PREC_BF16): weights as one bf16 each, one fragment per 16-channel
// k-step, so every layer has half the fragments of the 4-byte streams above.
constexpr int plain_f0(int l) {
    int f = 0;
    for (int i = 0; i < l; ++i) f += kLayerNT[i] * (kLayerKG[i] / 2);
    return f;
}
constexpr int kPlainUsedFrags = plain_f0(kNumLayers);                              // 1122
constexpr int kPlainNumSlices =
    ((kPlainUsedFrags + kSliceFrags - 1) / kSliceFrags + kRingSlots - 1) / kRingSlots * kRingSlots;  // 18
constexpr int kPlainStreamFrags = kPlainNumSlices * kSliceFrags;                   // 1152
static_assert(kPlainUsedFrags == 1122 && kPlainUsedFrags % 2 == 0, "plain stream table changed");

// Six-piece bf16 stream (IDN_PREC_BF16X6): per (n-tile, 16-channel k-step) a TRIPLE of fragments (p1, p2, p3) -- the three
// bf16 pieces of each weight.  Its ring slots hold 48 fragments = 16 k-steps, so slices, layer starts and ring phases sit on
// the same k-steps as in the 64-fragment rings above (16 k-steps of two fragments), and the stream is 3.375 MiB: it stays
// in a 4 MiB per-XCD L2.  (Round 2 padded every triple to a quad with a zero fragment: 4.5 MiB, 5 GB of fabric reads per
// launch where the other streams cause 43 MB.)
constexpr int kX6KFrags = 3;                                   // fragments per k-step
constexpr int kX6SliceFrags = 16 * kX6KFrags;                  // 48: one ring slot = 16 k-steps = 48 KiB
constexpr int kX6RingFrags = kRingSlots * kX6SliceFrags;       // 96 KiB ring
constexpr int kX6UsedFrags = kX6KFrags * kPlainUsedFrags;      // 3366
constexpr int kX6NumSlices = 2 * kNumSlices;                   // 72 (the same k-steps per slice as a quad stream had)
constexpr int kX6StreamFrags = kX6NumSlices * kX6SliceFrags;   // 3456 = 3.375 MiB
static_assert(kX6UsedFrags <= kX6StreamFrags && kX6StreamFrags - kX6UsedFrags < kX6RingFrags + kX6SliceFrags, "x6 stream table");

// Folded bias block: one float per output channel, natural channel order
// (accumulator register 4q+j of tile t, lane half h <-> channel 32 t + 8 q + 4 h + j).
constexpr int bias_off(int l) {
    int o = 0;
    for (int i = 0; i < l; ++i) o += kLayerNT[i] * 32;
    return o;
}
// ... followed by a copy of alpha_linear's weight row (256 floats): the fp32 kernel takes sigma as a
// 256-term dot product on the vector unit instead of a fifth 32-row MFMA tile of views_linears.0
// of which one row is used (1.6 % of the pass's MFMAs).
// and of rgb_linear's three weight rows (3 x 128): the same for the colour head (3 rows of 32 used).
constexpr int kAlphaOff = bias_off(kNumLayers);    // 2496
constexpr int kRgbOff = kAlphaOff + 256;           // 2752
constexpr int kBiasFloats = kRgbOff + 3 * 128;     // 3136
static_assert(kBiasFloats == 3136, "bias table changed");

// views0 carries sigma as channel 128 (tile 4, row 0): alpha_linear rides in the same
// pass over the trunk output instead of a separate N=1 layer.
constexpr int kSigmaChannel = 128;

// Colour gate (mlp_common.h): the longest sample spacing dist = (z[s+1] - z[s]) * |rays_d| across which a sample with
// sigma <= 0 is taken to have the weight exactly 0 (idealnerf_colour_gate_max_dist).
constexpr float kGateMaxDist = 0.0125f;

// ---------------------------------------------------------------------------
// Training-mode activation slab: layer-major row-major matrices of p_pad rows each
// (p_pad = n_points rounded up to 128; rows beyond n_points stay zero).
//   x0  [p_pad, 64]   gamma10(point), column 63 zero
//   dir [p_pad, 64]   gamma4(view dir) in columns 0..26, rest zero
//   a1..a8 [p_pad, 256]  post-ReLU outputs of pts_linears.0..7
//   v1..v3 [p_pad, 128]  post-ReLU outputs of views_linears.0..2
// act_off(i) = first column of matrix i when the slab is viewed as 2560 columns.
// ---------------------------------------------------------------------------
enum { kActX0 = 0, kActDir = 1, kActA1 = 2, kActV1 = 10, kActCount = 13 };
constexpr int act_width(int i) { return i < 2 ? 64 : (i < kActV1 ? 256 : 128); }
constexpr int act_off(int i) {
    int o = 0;
    for (int k = 0; k < i; ++k) o += act_width(k);
    return o;
}
constexpr int kActCols = act_off(kActCount);  // 2560
static_assert(kActCols == 2560, "activation slab layout changed");
// Behind the matrices: the ReLU masks of the 11 hidden layers as BITS, in the accumulator layout both MLP
// kernels share, so the backward delta chain loads one uint4 per lane and layer instead of gathering 16-byte
// pieces of the saved activations.  Layer id 0..7 = a1..a8, 8..10 = v1..v3; entry
// [id][wave tile = point / 32][lane] is a uint4 whose dword k holds tiles 2k, 2k+1: bit 31 - (16 (T & 1) + r)
// = 1 where the PRE-activation of register r of tile T is <= 0 (the unit is off; +0.0 counts as off, as in torch's relu backward).
constexpr int kMaskLayers = 11;
constexpr int kMaskFloatsPerPoint = kMaskLayers * 8;   // 2 lanes x 4 dwords per point and layer
constexpr int kActColsAll = kActCols + kMaskFloatsPerPoint;
__host__ __device__ inline size_t mask_index(int id, int64_t p_pad, int64_t wave_tile, int lane) {
    return ((size_t)id * (size_t)(p_pad / 32) + (size_t)wave_tile) * 64 + (size_t)lane;   // in uint4 units
}

// ---------------------------------------------------------------------------
// error plumbing (capi.hip)
// ---------------------------------------------------------------------------
int fail(int code, const char* fmt, ...);
#define IDN_HIP_CHECK(expr)                                                                   \
    do {                                                                                      \
        hipError_t _e = (expr);                                                               \
        if (_e != hipSuccess) return ::idn::fail(IDN_EHIP, "%s: %s", #expr, hipGetErrorString(_e)); \
    } while (0)

// ---------------------------------------------------------------------------
// Per-device launch state of a kernel family: the CU count (grid = min(tiles, CUs)) and the
// dynamic-LDS opt-in, done once per device under a lock.  The reference may run its model under
// nn.DataParallel (one host thread per device in ONE process): launches are
// re-entrant per device and stream.
// ---------------------------------------------------------------------------
struct LaunchSetup {
    static constexpr int kMaxDevices = 64;
    std::mutex mu;
    int cus[kMaxDevices] = {};
    template <class OptIn>
    int get(OptIn&& opt_in, int* num_cu) {
        int dev = 0;
        IDN_HIP_CHECK(hipGetDevice(&dev));
        if (dev < 0 || dev >= kMaxDevices) return ::idn::fail(IDN_EUNSUPPORTED, "device index %d out of range", dev);
        std::lock_guard<std::mutex> lock(mu);
        if (!cus[dev]) {
            hipDeviceProp_t prop;
            IDN_HIP_CHECK(hipGetDeviceProperties(&prop, dev));
            if (int e = opt_in()) return e;
            cus[dev] = prop.multiProcessorCount;
        }
        *num_cu = cus[dev];
        return IDN_OK;
    }
};

// ---------------------------------------------------------------------------
// optional per-launch timing of the MLP kernel (capi.hip); off by default
// ---------------------------------------------------------------------------
struct ProfScope {
    int slot;
    hipStream_t s;
    ProfScope(hipStream_t s, int64_t points, int kind = IDN_PROF_MLP_FWD);
    ~ProfScope();
};

// ---------------------------------------------------------------------------
// launchers (one per .hip file)
// ---------------------------------------------------------------------------
int launch_pack_f32(const idn_facenerf_params& p, float* packed, hipStream_t s);
int launch_pack_bf16x3(const idn_facenerf_params& p, float* packed, hipStream_t s, int fmt = 0);  // fmt 1: fp16 halves
int launch_pack_bf16x6(const idn_facenerf_params& p, float* packed, hipStream_t s);
int launch_pack_bf16(const idn_facenerf_params& p, float* packed, hipStream_t s);
int launch_fold(const idn_facenerf_params& p, const float* aud, const float* expr, const float* latent,
                float* folded, hipStream_t s);

// ---------------------------------------------------------------------------
// Network forward: the kernels' argument record IS the launchers' parameter.  The input mode is the pointer that is set:
// x (pre-embedded rows), pts (+ dirs), else rays + z.  A call site builds the record with the builder of its mode, so it
// names its mode and never writes another mode's pointers.
// ---------------------------------------------------------------------------
struct MlpArgs {
    const float* wstream;
    const float* bias;
    const float* x;     // kModeX:    [n_points, x_pts_ch + x_views_ch] pre-embedded rows
    const float* rays;  // kModeRays: [n_rays, 11]
    const float* z;     // kModeRays: [n_rays, S]
    const float* pts;   // kModePts:  [n_points, 3]
    const float* dirs;  // kModePts:  [n_rays, 3] unit view directions
    long n_points;
    int S;
    float* raw;         // [n_points, 4]
    float* acts;        // training only: activation slab (act_off() matrices of p_pad rows), else null
    long p_pad;
    int x_pts_ch, x_views_ch;   // the network's encoding widths (3..63, 3..27): kModeX reads rows of them; a saving launch of the
                                // other modes stores zeros in the slab's x0 / dir columns beyond them; else they are not read
};
// the colour-gated fp32 rays kernel's arguments (the other kernels' stay as they are)
struct MlpGateArgs : MlpArgs {
    unsigned long long* gate_counters;   // (tiles, skipped) this launch adds to, or null
    int tile_step;                       // tile_order_step(grid) (tile_order.h): the kernel's loop divides nothing
};
// both are copied into the kernarg segment as they are: a new field moves every kernel's argument layout
static_assert(sizeof(MlpArgs) == 104 && std::is_trivially_copyable<MlpArgs>::value, "kernel argument layout");
static_assert(sizeof(MlpGateArgs) == 120 && std::is_trivially_copyable<MlpGateArgs>::value, "kernel argument layout");

// what every mode sets; the pointers of the modes stay null, the widths at the default
inline MlpArgs mlp_no_input(const float* packed, const float* folded, int64_t n_points, int S, float* raw) {
    MlpArgs a = {};
    a.wstream = packed; a.bias = folded; a.n_points = (long)n_points; a.S = S; a.raw = raw;
    a.x_pts_ch = IDN_PTS_CH; a.x_views_ch = IDN_VIEWS_CH;
    return a;
}
inline MlpArgs mlp_rows(const float* packed, const float* folded, const float* x, int pts_ch, int views_ch, int64_t n, float* raw) {
    MlpArgs a = mlp_no_input(packed, folded, n, 1, raw);
    a.x = x; a.x_pts_ch = pts_ch; a.x_views_ch = views_ch;
    return a;
}
inline MlpArgs mlp_rays(const float* packed, const float* folded, const float* rays, const float* z, int64_t n_rays, int S, float* raw) {
    MlpArgs a = mlp_no_input(packed, folded, n_rays * S, S, raw);
    a.rays = rays; a.z = z;
    return a;
}
inline MlpArgs mlp_points(const float* packed, const float* folded, const float* pts, const float* dirs, int64_t n_rays, int S, float* raw) {
    MlpArgs a = mlp_no_input(packed, folded, n_rays * S, S, raw);
    a.pts = pts; a.dirs = dirs;
    return a;
}
// the training forward: the same launch also fills the activation slab (p_pad = n_points rounded up to 128)
inline MlpArgs mlp_saving(MlpArgs a, float* acts, int64_t p_pad) {
    a.acts = acts; a.p_pad = (long)p_pad;
    return a;
}
// ... of a rays- or pts-mode record for a network of these widths (mlp_rows carries its own)
inline MlpArgs mlp_saving(MlpArgs a, float* acts, int64_t p_pad, int pts_ch, int views_ch) {
    a.x_pts_ch = pts_ch; a.x_views_ch = views_ch;
    return mlp_saving(a, acts, p_pad);
}
// fp32 rays-mode inference only: the colour-gated kernel; counters: device int64 [2] (tiles, skipped) it adds to, or null
struct MlpGate { int on; int64_t* counters; };
// one launcher per arithmetic (mlp_launch.h holds their common body), and the precision dispatch in front of them.
// acts set: the training forward (IDN_PREC_F32 and IDN_PREC_BF16X6 build it).  The gate is the fp32 launcher's alone.
int launch_mlp_f32(const MlpArgs& a, hipStream_t s, MlpGate gate);
int launch_mlp_bf16x3(const MlpArgs& a, hipStream_t s);
int launch_mlp_fp16x3(const MlpArgs& a, hipStream_t s);
int launch_mlp_bf16(const MlpArgs& a, hipStream_t s);
int launch_mlp_bf16x6(const MlpArgs& a, hipStream_t s);
int launch_mlp(int precision, const MlpArgs& a, hipStream_t s, MlpGate gate);

int launch_frame_rays_pixels(const float* c2w_host, int H, int W, float focal, float cx, float cy, float near_, float far_,
                             int64_t pix0, int npix, float* rays_out, hipStream_t s);
size_t audio_net_saved_floats(int n);
int launch_audio_net_fwd(const idn_audio_net_params* p, const float* windows, int n, float* out, float* saved, hipStream_t s);
int launch_audio_net_bwd(const idn_audio_net_params* p, const idn_audio_net_grads* g, const float* windows, const float* saved,
                         const float* d_out, int n, hipStream_t s);
int launch_to8b(const float* rgb, int64_t n_pixels, int swap_rb, unsigned char* out, int* flag, hipStream_t s);
int launch_compose_to8b(const float* head, const float* lw, const float* fg, int64_t n_pixels, int swap_rb,
                        unsigned char* out, unsigned char* fg_out, int* flag, hipStream_t s);
// In-kernel draws (include/idealnerf.h: rng_mode): row `ray0 + r` of the Philox table replaces t_rand[r, :] / u[r, :]
struct Draws {
    unsigned long long seed;
    long ray0;
    int on;
};
int launch_philox_uniform(unsigned long long seed, int which, int64_t row0, int64_t n_rows, int n_cols, float* out, hipStream_t s);

// Render forward (composite.hip, render_fused.hip): as for the network, the kernels' argument records ARE the launchers'
// parameters, filled by name (SampleArgs and FusedArgs are copied into the kernarg segment as they are); the four input modes
// of the importance sampling have a builder each.
struct SampleArgs {
    const float* z;        // [n,S] coarse depths (null when bins_in is given)
    const float* weights;  // [n,S] (the kernel uses [:,1:-1]) or, with bins_in, [n,nb-1] as helper.sample_pdf takes them
    const float* cdf_in;   // [n,nb] optional: skip the pdf/cdf stage (bit-exact boundary)
    const float* bins_in;  // [n,nb]
    const float* u;
    int u_per_ray;
    long n_rays;
    int S, Ni, nb;
    float* z_samples;      // the outputs: a call site sets the ones it has, any may stay null
    int64_t* inds;
    float* cdf_out;
    float* z_fine;
    float* z_std;
    Draws draws;           // on: u is drawn here, row draws.ray0 + ray of the table (a.u is not read)
};
// what a compositing kernel reads; its outputs are the public idn_composite_out
struct CompositeIn {
    const float *raw, *z, *rays, *bc, *noise;   // noise [n,S]: added to sigma, or null
    int white_bkgd;
    int64_t n_rays;
    int S;
};
// the fused ray kernel (fp32, S = 64, Ni = 128)
struct FusedArgs {
    const float *wstream_c, *bias_c, *wstream_f, *bias_f;   // the packed weights and folded biases of the two networks
    const float *rays, *bc, *z_c, *u;   // [n, 11], [n, 3], [n, 64] coarse depths (coarse_depths_kernel), the importance draws
    int u_per_ray;
    long n_rays;
    int white_bkgd;
    idn_composite_out co, fo;   // outputs of the coarse / fine compositing, indexed by ray
    float* z_std;
    float *tap_raw_c, *tap_raw_f, *tap_z_fine;   // debug taps (any may be null)
    int64_t* tap_inds;
    float *tap_z_samples, *tap_cdf;
    float* z_f;          // [n, 192] fine depths in HBM: written by the coarse half, read by the fine half (split arrangement only)
    Draws draws;         // on: the importance draws come from the Philox table instead of `u`
};
static_assert(sizeof(SampleArgs) == 136 && std::is_trivially_copyable<SampleArgs>::value, "kernel argument layout");
static_assert(sizeof(FusedArgs) == 288 && std::is_trivially_copyable<FusedArgs>::value, "kernel argument layout");

// what every sampling mode sets: S - 1 bins, the inputs of the modes null, no in-kernel draws
inline SampleArgs sample_no_input(const float* u, int u_per_ray, int64_t n_rays, int S, int Ni) {
    SampleArgs a = {};
    a.u = u; a.u_per_ray = u_per_ray; a.n_rays = (long)n_rays; a.S = S; a.Ni = Ni; a.nb = S - 1;
    return a;
}
// bins = the midpoints of the coarse depths, weights[:, 1:-1] (idealnerf_sample_pdf_fwd)
inline SampleArgs sample_depths(const float* z, const float* weights, const float* u, int u_per_ray, int64_t n_rays, int S, int Ni) {
    SampleArgs a = sample_no_input(u, u_per_ray, n_rays, S, Ni);
    a.z = z; a.weights = weights;
    return a;
}
// the caller's own bins [n, n_bins] and interior weights [n, n_bins - 1] (idealnerf_sample_pdf_bins_fwd)
inline SampleArgs sample_bins(const float* bins, const float* weights, const float* u, int u_per_ray, int64_t n_rays, int n_bins, int Ni) {
    SampleArgs a = sample_no_input(u, u_per_ray, n_rays, n_bins + 1, Ni);
    a.bins_in = bins; a.weights = weights;
    return a;
}
// a given cdf [n, n_bins] over the bins: the inversion alone (idealnerf_invert_cdf)
inline SampleArgs sample_cdf(const float* cdf, const float* bins, const float* u, int u_per_ray, int64_t n_rays, int n_bins, int Ni) {
    SampleArgs a = sample_no_input(u, u_per_ray, n_rays, n_bins + 1, Ni);
    a.cdf_in = cdf; a.bins_in = bins;
    return a;
}
// the march: the rays and depths of `in`, whose compositing weights reach the sampling through LDS (weights stays null)
inline SampleArgs sample_march(const CompositeIn& in, const float* u, int u_per_ray, int Ni, Draws draws) {
    SampleArgs a = sample_no_input(u, u_per_ray, in.n_rays, in.S, Ni);
    a.z = in.z; a.draws = draws;
    return a;
}
int launch_coarse_depths(const float* rays, const float* t_vals, const float* t_rand, int64_t n_rays, int S,
                         int lindisp, float* z, Draws draws, hipStream_t s);
int launch_composite(const CompositeIn& in, const idn_composite_out& out, hipStream_t s);
// coarse raw2outputs + sample_pdf + merge in one kernel (the weights stay on chip); sample = sample_march(in, ...), which carries
// the depths, the ray count and S of `in`
int launch_march(const CompositeIn& in, const idn_composite_out& out, const SampleArgs& sample, hipStream_t s);
int launch_sample_pdf(const SampleArgs& sample, hipStream_t s);
// arrangement 1: coarse network -> march -> fine network -> compositing in ONE kernel;
// 2: coarse network + march | fine network + compositing (two launches, the fine depths a.z_f[n, 192] cross HBM between them)
int launch_render_fused(int arrangement, const FusedArgs& a, hipStream_t s);

// sampler.hip: the training loader's region-weighted pixel draw and the gather of the drawn pixels' rays / colours
int launch_sample_pixels(const unsigned char* map, int H, int W, const int counts[4], unsigned long long seed, unsigned long long draw,
                         int* population, long long* sel, hipStream_t s);
// (c2w2_host / batch_rays2: the optional second camera and its rays for the same pixels; nullptr = one camera)
int launch_gather_rays(const long long* sel, int64_t n, const float* c2w_host, const float* c2w2_host, int H, int W, float focal,
                       float cx, float cy, const unsigned char* image, const unsigned char* background, const float* target_table,
                       const float* background_table, float* batch_rays, float* batch_rays2, float* target_s, float* bc_rgb,
                       hipStream_t s);
// cull.hip: occupancy grid (mark, cells) and the per-frame ray cull (classify + compact, gather, fill + scatter)
int launch_cull_mark(const float* raw, int64_t n, float sigma_min, unsigned char* corners, hipStream_t s);
int launch_cull_cells(const unsigned char* corners, int G, int dilate, unsigned* bits, hipStream_t s);
size_t cull_classify_workspace_bytes(int64_t npix);
int launch_cull_classify(const idn_cull_grid& grid, const idn_frame& frame, float dz, int K, long long* sel, int* n_live, void* ws,
                         hipStream_t s);
int launch_cull_gather(const long long* sel, int64_t n, const idn_frame& frame, const float* bc, float* rays, float* bc_live,
                       hipStream_t s);
int launch_cull_scatter(const long long* sel, int64_t n_live, int64_t npix, const float* bc, const idn_cull_output* outs, int n_outs,
                        hipStream_t s);
// the sample cull of the live rays: classify + compact the points of z [n, S], gather their positions, scatter their outputs
int launch_cull_sample_classify(const idn_cull_grid& grid, const float* rays, const float* z, int64_t n_points, int S, long long* sel,
                                int* n_live, void* ws, hipStream_t s);
int launch_cull_sample_gather(const long long* sel, int64_t m, const float* rays, const float* z, int64_t n_points, int S, float* pts,
                              float* dirs, hipStream_t s);
int launch_cull_sample_scatter(const long long* sel, int64_t m, const float* raw_live, int64_t n_points, float* raw, hipStream_t s);
// metrics.hip: squared error and SSIM of a frame against its uint8 ground truth, whole frame and per region -> out [5, 4] fp64
size_t frame_scores_workspace_bytes(int H, int W);
int launch_frame_scores(const float* pred, const unsigned char* truth, const unsigned char* regions, int H, int W, double* out,
                        double* partial, hipStream_t s);
// ssim_loss.hip: the pixel indices of a set of patches, the patch SSIM loss -> out [n_patches + 1] fp64, and its gradient
int launch_patch_pixels(const idn_patch_set& set, int W, long long* sel, hipStream_t s);
int launch_ssim_patch_fwd(const float* pred, const float* truth, int n_patches, int p, double* out, hipStream_t s);
int launch_ssim_patch_bwd(const float* pred, const float* truth, int n_patches, int p, float g, float* d_pred, hipStream_t s);

// ---------------------------------------------------------------------------
// Backward delta chain (mlp_f32_bwd.hip): the transposed weights as a second fragment stream.
// Stage s computes D_in^T = W_s^T . D_out^T for 32 points per wave, masks it with the layer's
// packed ReLU bits and keeps it in registers as the next stage's B operand.
//   0 rgb_linear^T (K 3, padded)   1 views_linears.2^T   2 views_linears.1^T
//   3 views_linears.0[:, :256]^T + alpha_linear^T as k-channel 128 (K 129, padded)
//   4..10 pts_linears.7 .. pts_linears.1 ^T (pts_linears.5: its 256 hidden columns)
// Stages 0-3 end at fragment 280; the stream is padded to 384 so that every 256-fragment trunk
// stage starts on the same ring phase (one loop body serves them all).
// ---------------------------------------------------------------------------
constexpr int kBwdStages = 11;
constexpr int kBwdNT[kBwdStages] = {4, 4, 4, 8, 8, 8, 8, 8, 8, 8, 8};
constexpr int kBwdKG[kBwdStages] = {2, 16, 16, 18, 32, 32, 32, 32, 32, 32, 32};
constexpr int kBwdHeadFrags = 280, kBwdTrunk0 = 384;
constexpr int bwd_f0(int s) {
    if (s >= 4) return kBwdTrunk0 + 256 * (s - 4);
    int f = 0;
    for (int i = 0; i < s; ++i) f += kBwdNT[i] * kBwdKG[i];
    return f;
}
static_assert(bwd_f0(3) + kBwdNT[3] * kBwdKG[3] == kBwdHeadFrags, "head stages");
constexpr int kBwdStreamFrags = kBwdTrunk0 + 7 * 256;   // 2176
static_assert(kBwdStreamFrags % kSliceFrags == 0 && kBwdTrunk0 % kRingFrags == 0, "ring phase of the trunk stages");
constexpr int kBwdNumSlices = kBwdStreamFrags / kSliceFrags;

int launch_pack_f32_bwd(const idn_facenerf_params& p, float* packed_bwd, hipStream_t s);
// d_rgb: [p_pad, 64] (cols 0..2 = d raw rgb), dv0: [p_pad, 256] (col 128 = d raw sigma; cols 0..127 are written),
// acts: the forward's activation slab, dv2/dv1: [p_pad, 128], da[l]: [p_pad, 256] = delta of pts_linears.l
int launch_delta_chain(const float* packed_bwd, const float* acts, int64_t p_pad, const float* d_rgb, float* dv0,
                       float* dv2, float* dv1, float* const da[8], hipStream_t s, int max_grid = 0,
                       int* grid_out = nullptr);   // max_grid > 0 caps the grid; grid_out: the grid that was launched
// the same chain as six bf16 piece products per fp32 product (its own transposed stream, twice the fragments)
size_t bwd_stream_floats_x6();
int launch_pack_bf16x6_bwd(const idn_facenerf_params& p, float* packed_bwd, hipStream_t s);
int launch_delta_chain_x6(const float* packed_bwd, const float* acts, int64_t p_pad, const float* d_rgb, float* dv0,
                          float* dv2, float* dv1, float* const da[8], hipStream_t s, int max_grid = 0,
                          int* grid_out = nullptr);
// the chain alone, as bwd_tail launches it for `pipe` (idealnerf_delta_chain); da: [8][p_pad, 256], dv21: [p_pad, 256]
size_t delta_chain_workspace_bytes();
int launch_delta_chain_alone(const idn_facenerf_params& p, int pipe, const float* acts, int64_t p_pad, const float* d_rgb,
                             float* dv0, float* dv21, float* da, int max_blocks, int* blocks_out, void* ws, size_t ws_bytes,
                             hipStream_t s);

// dw_gemm.hip: one 256 x 256 weight-gradient product in isolation (idealnerf_dw_gemm); pipe: IDN_DW_PIPE_*
size_t dw_gemm_workspace_bytes();
int launch_dw_gemm(const float* delta, int ld_delta, const float* acts, int ld_acts, int64_t rows, float* dW, float* db, int pipe,
                   void* ws, size_t ws_bytes, hipStream_t s);
// a list of products of any of the pass's shapes through one pass plan (idealnerf_dw_products)
size_t dw_products_workspace_bytes();
int launch_dw_products(int64_t rows, int pipe, int x6_items, idn_dw_product* products, int n, void* ws, size_t ws_bytes, hipStream_t s);

// train.hip: backward of one render pass
size_t bwd_workspace_bytes(int64_t n_points);
// the conditioning vectors of a network and where a backward puts their gradients (a null gradient is not delivered)
struct BwdCond {
    const float *aud, *expr, *latent;
    float *d_aud, *d_expr, *d_latent;   // d_expr [dim_expr]: accumulated
    float* d_vb;                        // [128], the frozen plan only: views_linears.0's bias gradient, overwritten
};
// One pass backward, as the four idealnerf_pass_bwd* entries fill it; a field an entry does not have stays null.
struct PassBwd {
    const idn_facenerf_params* p;
    const idn_facenerf_grads* grads;    // null: the conditioning-only plan of a frozen network (no gradient tensor is written)
    BwdCond cond;
    const float *acts, *raw, *z, *rays, *bc;
    int64_t n_rays;
    int S;
    const float *g_rgb, *g_fg, *g_lw, *g_acc;   // the gradients of the pass's four outputs
    float* d_rays;                      // [n_rays, 11] != null: also the gradient of the ray records (overwritten)
    void* ws;
    size_t ws_bytes;
};
int launch_pass_bwd(const PassBwd& b, hipStream_t s);
// The compositing backward, d(rgb_map, rgb_fg, last_weight, acc) -> d raw: the first launch of launch_pass_bwd, which calls this
// function, and all of idealnerf_composite_bwd.
struct CompBwdArgs {
    const float4* raw; const float* z; const float* rays; const float* bc;
    const float* g_rgb;  // [n,3] d rgb_map (may be null)
    const float* g_fg;   // [n,3] d rgb_fg  (may be null)
    const float* g_lw;   // [n]   d last_weight (may be null)
    const float* g_acc;  // [n]   d acc_map (may be null)
    float* d_rgb; int ld_rgb;    // row p = ray*S+s: d raw_rgb at d_rgb[p*ld_rgb + 0..2]
    float* d_sig; int ld_sig;    // d raw_sigma at d_sig[p*ld_sig]
    long n_rays; int S;
    float* d_norm; int ld_norm;  // kNorm kernels only: dL / d |rays_d| = sum_{s < S-1} (dL / d dist_s) (z_{s+1} - z_s) at d_norm[ray*ld_norm]
};
// S outside [2, 512]: IDN_EUNSUPPORTED.  d_norm null: the kernels without the |rays_d| gradient.
int launch_composite_bwd(const CompBwdArgs& a, hipStream_t s);
// ray_grad.hip: d_x [n_rays * S, pts_ch + views_ch] (the input-row gradient of the pass's points) -> d_rays [n_rays, 11];
// column 6 of d_rays holds dL / d |rays_d| on entry
int launch_ray_grad(const float* d_x, int pts_ch, int views_ch, const float* rays, const float* z, int64_t n_rays, int S,
                    float* d_rays, hipStream_t s);
// train.hip: the stages of a backward that follow the delta chain, each as the pass launches it and as its test aid does
// (idealnerf_input_grad, idealnerf_fold_bwd, idealnerf_cond_colsums).
// d_x [n, pts_ch + views_ch] from the three [Pp, 256] delta matrices dA[0], dA[5], dV0.  max_blocks 0: the grid of a pass;
// k > 0 caps it at k workgroups; blocks_out (may be null): the grid that ran
int launch_dx(const idn_facenerf_params& p, const float* dA0, const float* dA5, const float* dV0, int64_t n, int64_t Pp, float* d_x,
              int max_blocks, int* blocks_out, hipStream_t s);
struct FoldBwdArgs {
    idn_facenerf_params p;
    const float* aud; const float* expr; const float* latent;
    const float* db0; const float* db5; const float* dbv;  // [256], [256], [128]
    float* gW0; float* gW5; float* gWv0;                    // gradient tensors (full nn.Linear layout)
    float* d_aud; float* d_latent;                          // accumulated (+=), may be null
    float* d_expr;                                          // accumulated (+=), may be null (the expression takes no gradient)
};
// cond_only: the d cond range alone, gW0 / gW5 / gWv0 are not touched (a frozen network)
int launch_fold_bwd(const FoldBwdArgs& f, bool cond_only, hipStream_t s);
// db [2][256] = column sums of dA0 | dA5 over Pp rows (dA0 null: left out), dbv [128] = those of dV0[:, 0:128] over the first
// P rows (dV0 null: left out); part: cond_colsums_workspace_bytes() bytes
size_t cond_colsums_workspace_bytes();
int launch_cond_colsums(const float* dA0, const float* dA5, const float* dV0, int64_t P, int64_t Pp, float* db, float* dbv,
                        double* part, hipStream_t s);
// FaceNeRF.forward's backward on pre-embedded rows: head deltas from g_out [n, 4], the same tail as launch_pass_bwd, d expr
// from the fold and (d_x != null) the input-row gradient d_x [n, pts_ch + views_ch]
int launch_facenerf_bwd(const idn_facenerf_params& p, const idn_facenerf_grads& gr, const BwdCond& cond, const float* acts,
                        int64_t n, const float* g_out, float* d_x, void* ws, size_t ws_bytes, hipStream_t s);

}  // namespace idn
