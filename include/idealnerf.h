/*
 * idealnerf.h -- C ABI of libidealnerf.so, the MI355X (gfx950) implementation of
 * IDEAL-NeRF's per-ray hot path.
 *
 * The reference (GaryGky/IDEAL-NeRF) is pure Python and has no FFI of its own; its
 * seam for this path is the set of Python callables listed beside each entry point
 * below (paths relative to the reference root).  The Python host layer in
 * ideal-nerf_amd/ mirrors those callables and binds this header through ctypes
 * (see INTEGRATION.md for the stub a reference maintainer would add).
 *
 * Conventions
 *   - every pointer is a DEVICE pointer to contiguous row-major memory owned by the
 *     caller (fp32 unless stated; indices int64), except where marked [host];
 *   - `stream` is a hipStream_t passed as void*; calls enqueue work and return, they
 *     never synchronise, allocate or free;
 *   - return 0 on success, a negative IDN_E* code otherwise; idealnerf_last_error()
 *     returns a thread-local message for the last failure on the calling thread;
 *   - no global mutable state: calls on different streams/devices are independent
 *     (the reference's nn.DataParallel replicas call forward concurrently,
 *     NeRFs/HeadNeRF/test/eval_aud_exp_nerf.py:475).
 *
 * Network architecture is the reference's: D=8, W=256, skips=[4], use_viewdirs=True
 * (NeRFs/HeadNeRF/train/audio_exp_nerf.py:213-224).  The encoding widths are a property of
 * the network: multires in 0..10 (3 + 6 multires point channels, 63 at the default 10) and
 * multires_views in 0..4 (3 + 6 multires_views direction channels, 27 at the default 4), as
 * helper.get_embedder gives them (helper.py:174-224; i_embed = -1 is 0 / 0).  gamma_L is a
 * prefix of gamma_10: a narrower network's weight stream holds zeros in the columns it does
 * not have, and the ray / point kernels evaluate the full encoding against them.  The
 * conditioning widths (dim_aud, dim_expr, dim_latent) are free: they only enter the
 * per-frame folded biases.  Other architectures are rejected with IDN_EUNSUPPORTED.
 */
#ifndef IDEALNERF_H
#define IDEALNERF_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define IDN_OK 0
#define IDN_EINVAL (-1)       /* bad argument (null pointer, bad size) */
#define IDN_EUNSUPPORTED (-2) /* architecture / size outside the compiled path */
#define IDN_EHIP (-3)         /* a HIP runtime call failed (message has the code) */
#define IDN_EWORKSPACE (-4)   /* workspace too small */

/* Fixed architecture constants (models/face_nerf.py:9-37 at the reference's flags). */
#define IDN_W 256
#define IDN_D 8
#define IDN_PTS_CH 63   /* the widest point encoding (multires 10): the compiled 64-column input tile */
#define IDN_VIEWS_CH 27 /* the widest direction encoding (multires_views 4): the compiled 32-column input tile */
#define IDN_MAX_MULTIRES 10
#define IDN_MAX_MULTIRES_VIEWS 4
#define IDN_RAY_FLOATS 11 /* o(3) d(3) near far viewdir(3): audio_exp_nerf.py:412-427 */

/* Arithmetic of the MLP contraction. */
#define IDN_PREC_F32 0    /* v_mfma_f32_32x32x2_f32: exact fp32 fma chains */
#define IDN_PREC_BF16X3 1 /* 3 bf16 MFMAs per product (hi*hi + hi*lo + lo*hi), fp32 accumulate */
#define IDN_PREC_BF16 2   /* plain bf16 MFMA, fp32 accumulate (BASELINE config 5 only) */
#define IDN_PREC_FP16X3 3 /* 3 fp16 MFMAs per product (11+11 significand bits per operand): ~5e-7 on the
                             network output at the bf16x3 speed; activations must stay below 6.5e4 */
#define IDN_PREC_BF16X6 4 /* 6 bf16 MFMAs per product: weights and activations as the exact sum of three bf16 pieces
                             (24 significand bits, fp32's range), fp32 accumulate: fp32-grade (error <= 2^-23 per product) */

int idealnerf_version(void);
const char* idealnerf_last_error(void);

/* Sizes (in floats) of the two per-network device buffers the kernels consume. */
size_t idealnerf_packed_weight_floats(int precision);
size_t idealnerf_folded_bias_floats(void);

/*
 * The 24 parameter tensors of one FaceNeRF in state_dict order, nn.Linear layout
 * [out, in] (models/face_nerf.py:27-37):
 *   pts_w[i]/pts_b[i], i=0..7      pts_linears.i.{weight,bias}
 *   views_w[i]/views_b[i], i=0..2  views_linears.i.{weight,bias}
 *   alpha_w/alpha_b                alpha_linear.{weight,bias}
 *   rgb_w/rgb_b                    rgb_linear.{weight,bias}
 * feature_linear.* exists in the state_dict but is never applied (face_nerf.py:34 vs :66)
 * and is therefore not part of this struct.
 */
typedef struct idn_facenerf_params {
    const float* pts_w[8];
    const float* pts_b[8];
    const float* views_w[3];
    const float* views_b[3];
    const float* alpha_w;
    const float* alpha_b;
    const float* rgb_w;
    const float* rgb_b;
    int dim_aud, dim_expr, dim_latent; /* widths of the per-frame conditioning vectors */
    /* Encoding widths, stored as the value + 1 so that a zero-initialised struct means the defaults:
     * 0 = multires 10 / multires_views 4; otherwise multires + 1 in 1..11, multires_views + 1 in 1..5.
     * pts_linears.0 / .5 then have 3 + 6 multires encoding columns in front of the conditioning columns and
     * views_linears.0 has 3 + 6 multires_views direction columns behind its 256 trunk columns; every gradient
     * tensor has its parameter's (narrower) shape.  Anything else returns IDN_EINVAL. */
    int multires_plus1, multires_views_plus1;
} idn_facenerf_params;

/* The widths a params struct names (63 / 27 for a zero-initialised one), or -1 for a value out of range. */
int idealnerf_params_pts_ch(const idn_facenerf_params* p);
int idealnerf_params_views_ch(const idn_facenerf_params* p);

/*
 * Re-lay the per-point part of the weights into MFMA-fragment order
 * (`packed`, idealnerf_packed_weight_floats() floats).  Run once per weight update.
 * Replaces nothing in the reference; it is the load-time half of
 * FaceNeRF.forward (models/face_nerf.py:40-80).
 */
int idealnerf_pack_weights(const idn_facenerf_params* p, int precision, float* packed, void* stream);

/*
 * Fold the per-frame conditioning vectors into bias vectors
 * (`folded`, idealnerf_folded_bias_floats() floats):
 *   b0' = b0 + W0[:, 63:]  . [aud | expr/3 | latent]        (face_nerf.py:45-55,58)
 *   b5' = b5 + W5[:, 63:63+C] . [aud | expr/3 | latent]     (face_nerf.py:61)
 *   bv' = bv + Wv0[:, 283:] . expr/3                        (face_nerf.py:68-70)
 * (63 and 283 = 256 + 27 at the default widths; pts_ch and 256 + views_ch of the network otherwise)
 * aud / expr / latent may be NULL exactly when their width is 0 (or, for expr and
 * latent, when the caller passes None as the reference allows).  Run once per frame.
 */
int idealnerf_fold_conditioning(const idn_facenerf_params* p, const float* aud, const float* expr,
                                const float* latent, float* folded, void* stream);

/*
 * FaceNeRF.forward (models/face_nerf.py:40-80): x[n, 90] = [gamma10(pts) | gamma4(dir)]
 * -> out[n, 4] = (rgb_raw, sigma_raw).
 */
int idealnerf_facenerf_fwd(const float* packed, const float* folded, int precision, const float* x,
                           int64_t n, float* out, void* stream);
/* The same for a network of other encoding widths: x[n, pts_ch + views_ch], pts_ch = 3 + 6 multires (3..63),
 * views_ch = 3 + 6 multires_views (3..27); `packed` must come from a params struct of those widths.  The entry above
 * is this one at 63 / 27.  A width outside the range returns IDN_EINVAL before any launch.  Additive entry: the ABI
 * version is unchanged. */
int idealnerf_facenerf_fwd_ch(const float* packed, const float* folded, int precision, const float* x, int pts_ch,
                              int views_ch, int64_t n, float* out, void* stream);

/*
 * Network.run_network with the embedders fused (audio_exp_nerf.py:376-394 +
 * helper.py:174-224): for ray r and sample s, point = o_r + d_r * z[r, s] is
 * encoded in registers and evaluated; raw[r, s, :] = (rgb_raw, sigma_raw).
 */
int idealnerf_query_rays_fwd(const float* packed, const float* folded, int precision, const float* rays,
                             const float* z, int64_t n_rays, int n_samples, float* raw, void* stream);

/* Same, for callers that hold the sample points themselves (the literal signature of
 * Network.run_network, audio_exp_nerf.py:376): pts[n_rays, n_samples, 3],
 * viewdirs[n_rays, 3] (unit vectors, one per ray). */
int idealnerf_query_points_fwd(const float* packed, const float* folded, int precision, const float* pts,
                               const float* viewdirs, int64_t n_rays, int n_samples, float* raw, void* stream);

/* get_rays + ray-record assembly for rows [row0, row0+nrows) of an HxW frame
 * (helper.py:228-243, audio_exp_nerf.py:396-427; default principal point W/2,H/2 when
 * cx/cy < 0).  c2w is 12 floats, row-major [3,4], [host] memory.  rays_out[nrows*W, 11]. */
int idealnerf_frame_rays(const float* c2w, int H, int W, float focal, float cx, float cy, float near_, float far_,
                         int row0, int nrows, float* rays_out, void* stream);

/* Coarse depths (audio_exp_nerf.py:306-330): z[r,s] = near_r (1-t_s) + far_r t_s -- or, with
 * lindisp != 0, linear in inverse depth: 1 / ((1/near_r)(1-t_s) + (1/far_r) t_s) (:309-310) -- with
 * optional stratified jitter from t_rand[n_rays, n_samples] (NULL = perturb 0).
 * t_vals[n_samples] is the caller's torch.linspace(0,1,S) buffer. */
int idealnerf_coarse_depths(const float* rays, const float* t_vals, const float* t_rand, int lindisp, int64_t n_rays,
                            int n_samples, float* z, void* stream);

/*
 * raw2outputs (NeRFs/HeadNeRF/train/baseline.py:325-375; rgb_fg: NeRFs/TorsoNeRF/run_nerf.py:757).
 * Any output pointer may be NULL.  weights[n_rays, n_samples].
 */
typedef struct idn_composite_out {
    float* rgb_map;   /* [n,3] */
    float* disp_map;  /* [n]   */
    float* acc_map;   /* [n]   */
    float* depth_map; /* [n]   */
    float* weights;   /* [n,S] */
    float* rgb_fg;    /* [n,3] */
    float* last_weight; /* [n] = weights[:, -1] */
} idn_composite_out;

/* sigma_noise[n_rays, n_samples] (may be NULL) is added to the raw density before its ReLU: the caller draws
 * it as the reference does, randn * raw_noise_std (baseline.py:353-361).  white_bkgd != 0 adds 1 - acc_map to
 * rgb_map (:372-373).  The reference's Network never enables either (audio_exp_nerf.py:297-299). */
int idealnerf_composite_fwd(const float* raw, const float* z, const float* rays, const float* bc_rgb,
                            const float* sigma_noise, int white_bkgd, int64_t n_rays, int n_samples,
                            const idn_composite_out* out, void* stream);

/*
 * sample_pdf + merge (helper.py:269-313, audio_exp_nerf.py:340-349).
 *   weights[n, S] are the coarse compositing weights; the kernel uses weights[:, 1:-1]
 *   and bins = midpoints of z[n, S].
 *   u: [n_importance] shared by all rays when u_per_ray == 0 (deterministic,
 *      torch.linspace buffer), or [n, n_importance] when u_per_ray != 0.
 * Outputs (each may be NULL): z_samples[n, Ni], inds[n, Ni] (int64, searchsorted
 * right=True result), cdf[n, S-1], z_fine[n, S+Ni] (sorted union), z_std[n].
 * For identical weights in, cdf and inds are bit-identical to the reference's CPU path: the
 * normalising torch.sum is evaluated in ATen's own order (8 vector lanes, 4 accumulators), the
 * cumsum in fp64 rounded per element.
 */
int idealnerf_sample_pdf_fwd(const float* z, const float* weights, const float* u, int u_per_ray,
                             int64_t n_rays, int n_samples, int n_importance, float* z_samples, int64_t* inds,
                             float* cdf, float* z_fine, float* z_std, void* stream);

/*
 * The ray march between the two network passes as one kernel (audio_exp_nerf.py:335-349): raw2outputs of the
 * coarse pass, sample_pdf on its weights and the sorted merge with the coarse depths, one wavefront per ray.
 * Same arithmetic and outputs as idealnerf_composite_fwd followed by idealnerf_sample_pdf_fwd (bit for bit),
 * but the [n, S] weight matrix stays in LDS: out->weights is written only if it is not NULL.
 * idealnerf_render_rays_fwd uses it for every render with n_importance > 0.
 */
int idealnerf_march_fwd(const float* raw, const float* z, const float* rays, const float* bc_rgb, const float* sigma_noise,
                        int white_bkgd, const float* u, int u_per_ray, int64_t n_rays, int n_samples, int n_importance,
                        const idn_composite_out* out, float* z_samples, int64_t* inds, float* cdf, float* z_fine,
                        float* z_std, void* stream);

/* helper.sample_pdf with its own argument list (NeRFs/HeadNeRF/helper.py:269-313): bins[n, n_bins],
 * weights[n, n_bins-1] (the interior weights as the caller sliced them, before the +1e-5), u as above
 * -> z_samples[n, Ni], inds[n, Ni], cdf[n, n_bins] (each may be NULL).  Same kernel, same pdf / cdf
 * arithmetic as idealnerf_sample_pdf_fwd: torch.sum in ATen's CPU order, cumsum in fp64. */
int idealnerf_sample_pdf_bins_fwd(const float* bins, const float* weights, const float* u, int u_per_ray,
                                  int64_t n_rays, int n_bins, int n_importance, float* z_samples, int64_t* inds,
                                  float* cdf, void* stream);

/* The bit-exact boundary on its own (helper.py:297-310): given cdf[n, nb], bins[n, nb],
 * u (as above) -> inds (int64) and z_samples. */
int idealnerf_invert_cdf(const float* cdf, const float* bins, const float* u, int u_per_ray, int64_t n_rays,
                         int n_bins, int n_importance, float* z_samples, int64_t* inds, void* stream);

/*
 * Network.render_rays forward (audio_exp_nerf.py:297-371), all stages on `stream`.
 */
typedef struct idn_render_args {
    const float* rays;    /* [n,11] */
    const float* bc_rgb;  /* [n,3]  */
    int64_t n_rays;
    int n_samples;        /* N_samples   (2..256)  */
    int n_importance;     /* N_importance (0..256) */
    int precision;
    const float* packed_coarse;
    const float* folded_coarse;
    const float* packed_fine;   /* may be NULL when n_importance == 0 */
    const float* folded_fine;
    const float* t_vals;  /* [n_samples] torch.linspace(0,1,N_samples) */
    const float* t_rand;  /* [n, n_samples] or NULL (perturb == 0, or rng_mode == 1) */
    const float* u;       /* [n_importance] (u_per_ray=0) or [n, n_importance]; NULL with rng_mode == 1 */
    int u_per_ray;
    /* outputs, any may be NULL */
    float* rgb_map;  float* disp_map;  float* acc_map;  float* depth_map;  float* last_weight;  float* rgb_fg;
    float* rgb0;     float* disp0;     float* acc0;     float* z_std;      float* last_weight0; float* rgb_fg0;
    /* debug taps, any may be NULL */
    float* tap_z_coarse;   /* [n,S]     */
    float* tap_raw_coarse; /* [n,S,4]   */
    float* tap_weights_coarse; /* [n,S] */
    float* tap_cdf;        /* [n,S-1]   */
    int64_t* tap_inds;     /* [n,Ni]    */
    float* tap_z_samples;  /* [n,Ni]    */
    float* tap_z_fine;     /* [n,S+Ni]  */
    float* tap_raw_fine;   /* [n,S+Ni,4]*/
    float* tap_weights_fine; /* [n,S+Ni]*/
    void* workspace;       /* idealnerf_render_workspace_bytes() bytes */
    size_t workspace_bytes;
    /* Arithmetic of the FINE network's launches: 0 = same as `precision`, else IDN_PREC_* + 1.
     * "mixed" rendering = precision IDN_PREC_F32 with precision_fine_plus1 = IDN_PREC_BF16X3 + 1: the
     * coarse pass, whose output drives the importance sampling (which amplifies arithmetic noise), stays
     * exact; the fine pass (3/4 of the samples, nothing sampled after it) runs at the bf16 matrix rate.
     * packed_fine must have been packed for that arithmetic. */
    int precision_fine_plus1;
    /* render_rays' remaining switches (audio_exp_nerf.py:297-299; the reference leaves them at their defaults) */
    int lindisp;               /* coarse depths linear in inverse depth */
    int white_bkgd;            /* rgb += 1 - acc, in both passes */
    const float* noise_coarse; /* [n, n_samples] or NULL: raw_noise_std noise of the coarse pass, drawn by the caller */
    const float* noise_fine;   /* [n, n_samples + n_importance] or NULL */
    /* 0: the kernel sequence (network, march, network, compositing; raw outputs and fine depths through HBM).
     * 1: the whole per-ray path as ONE kernel that keeps a ray's sample positions, raw network outputs, weights and cdf in
     *    LDS -- nothing per-sample crosses HBM (csrc/render_fused.hip); 0-0.5 % faster than the sequence on a full frame, but it
     *    re-fetches a network's weight stream into every L2 at each change of network (six times the sequence's HBM bytes).
     * 2: the same kernel as two launches -- coarse network + march | fine network + compositing: one network per launch,
     *    so the weight stream stays in L2, and only the 768 bytes of fine depths per ray cross HBM between the launches
     *    (half the sequence's HBM bytes, 0.5 % slower).
     * 1 and 2 give the sequence's results bit for bit; they are built for the fp32 arithmetic at n_samples = 64,
     * n_importance = 128 without density noise (anything else returns IDN_EUNSUPPORTED).  DESIGN.md section 3. */
    int fused_march;
    /* The reference's perturb > 0 draws made inside the kernels instead of handed over as tensors ("optional
     * t_rand / u buffers or Philox seed").  rng_mode = 1: t_rand and u must be NULL; ray r of this call (counted from rng_ray0, so
     * that the chunks, row bands or ranks of one frame draw from ONE table whatever the partition) uses
     *   t_rand[r, s] = idealnerf_philox_uniform's value (which = 0, row rng_ray0 + r, column s)   -- torch.rand(z_vals.shape),
     *                                                                                                 audio_exp_nerf.py:314-326
     *   u[r, j]      = ... (which = 1, row rng_ray0 + r, column j)                                 -- torch.rand(.., N_samples),
     *                                                                                                 helper.py:283
     * in the kernels that consume them (coarse depths; inverse CDF of the march / the fused ray kernel): no [n, S] / [n, Ni]
     * random tensor exists.  Same distribution as torch.rand (24-bit uniform on [0, 1)); the NUMBERS are this library's own
     * (upstream's CUDA generator is no contract either: its numbers depend on its launch geometry). */
    int rng_mode;
    uint64_t rng_seed;
    int64_t rng_ray0;
} idn_render_args;

/* The table rng_mode = 1 draws from, as a tensor -- stands where upstream calls torch.rand for `t_rand` (audio_exp_nerf.py:314-326)
 * and `u` (helper.py:283); for the stand-alone entries, which take t_rand / u as tensors, and for checking:
 * out[r, c] (r < n_rows, c < n_cols) = the 24-bit uniform ((x >> 8) * 2^-24) of word c % 4 of Philox4x32-10 (Salmon et al., SC'11;
 * ten rounds, multipliers 0xD2511F53 / 0xCD9E8D57, key increments 0x9E3779B9 / 0xBB67AE85) with key = (seed low, seed high) and
 * counter = (c / 4, 0, low, high of 2 * (row0 + r) + which).  which: 0 = stratified offsets (t_rand), 1 = importance draws (u). */
int idealnerf_philox_uniform(uint64_t seed, int which, int64_t row0, int64_t n_rows, int n_cols, float* out, void* stream);

/*
 * The training loader's ray sampler on the device: GetData.sample_rays (NeRFs/HeadNeRF/train/audio_exp_nerf.py:134-195) as two
 * launches, with no host round trip and no full-frame ray tensor.  Additive entries: the ABI version is unchanged.
 *
 * idealnerf_sample_pixels: region_map is uint8 [H, W]; bit 0 = face rect minus mouth box, bit 1 = outside the face rect,
 * bit 2 = mouth box, bit 3 = torso (a pixel may carry bit 3 beside another).  sel receives n_rect + n_outside + n_mouth + n_torso
 * flat row-major pixel indices in the reference's order: rect, outside, mouth, torso (:143-187).
 *
 * Sampling without replacement is DEFINED, so that it can be checked exactly.  For region g in {0 rect, 1 outside, 2 mouth,
 * 3 torso} and flat pixel p, key(p, g) = word 0 of Philox4x32-10 (the generator of idealnerf_philox_uniform) with
 * key = (seed low, seed high) and counter = (p, g, draw low, draw high).  Region g contributes its c_g pixels with the smallest
 * (key, p) pairs, in ascending (key, p) order: keys are independent and uniform, so this is a uniform c_g-subset in uniform random
 * order -- the distribution of np.random.choice(replace=False).  Regions are drawn independently, as upstream.
 * The result is a function of (region_map, counts, seed, draw) alone: launch geometry and scheduling do not enter.
 *
 * A per-region count above IDN_SAMPLE_MAX_REGION returns IDN_EUNSUPPORTED (nothing is truncated).  A count above the region's
 * population cannot be seen from the host without a device read: the caller knows its populations (dataset.ResidentFrames checks
 * them at load time); if it happens all the same, that region's rows of sel are -1, which idealnerf_gather_rays turns into zero
 * rows.  workspace: idealnerf_sample_pixels_workspace_bytes() bytes, int32-aligned; on return (in stream order) its first four
 * int32 hold each region's population as the kernel counted it (-1 for a region whose count is 0: not counted).
 */
#define IDN_SAMPLE_MAX_REGION 4096 /* largest per-region count; the reference's default split needs 2675 (N_rand 3072, mouth 256, rate 0.95) */
size_t idealnerf_sample_pixels_workspace_bytes(void);
int idealnerf_sample_pixels(const uint8_t* region_map, int H, int W, int n_rect, int n_outside, int n_mouth, int n_torso,
                            uint64_t seed, uint64_t draw, void* workspace, size_t workspace_bytes, int64_t* sel, void* stream);

/*
 * idealnerf_gather_rays: for the n pixels of sel, batch_rays [2, n, 3] (origins, then UNNORMALISED directions: columns 0:3 and
 * 3:6 of the rows idealnerf_frame_rays writes for those pixels, bit for bit -- same operations, same order), target_s [n, 3] =
 * target_table[image[p]] and bc_rgb [n, 3] = background_table[background[p]].  c2w [host]: 12 floats, the [3, 4] camera matrix;
 * cx / cy < 0: the frame centre, as in idealnerf_frame_rays.  image / background: uint8 [H, W, 3].  The two tables are fp32 [256]
 * on the device: what a byte becomes (the loader's `uint8 -> float32 / 255` for the target, `float64 / 255` rounded to fp32 for
 * the background), built once by the caller so that the values are the loader's own.  Rows of sel outside [0, H W) give zeros.
 */
int idealnerf_gather_rays(const int64_t* sel, int64_t n, const float* c2w, int H, int W, float focal, float cx, float cy,
                          const uint8_t* image, const uint8_t* background, const float* target_table, const float* background_table,
                          float* batch_rays, float* target_s, float* bc_rgb, void* stream);

/*
 * idealnerf_gather_ray_pairs: idealnerf_gather_rays with a second camera for the same pixels, in the same launch -- the torso
 * stage's loader (NeRFs/TorsoNeRF/train_torso.py:130-183), whose batch_rays_torso are the selected pixels seen from the clip's
 * frame-0 pose.  batch_rays_torso [2, n, 3] comes from c2w_torso by the same operations in the same order as batch_rays from
 * c2w: each equals what idealnerf_gather_rays writes for that camera, bit for bit.  Additive entry: the ABI version is unchanged.
 */
int idealnerf_gather_ray_pairs(const int64_t* sel, int64_t n, const float* c2w, const float* c2w_torso, int H, int W, float focal,
                               float cx, float cy, const uint8_t* image, const uint8_t* background, const float* target_table,
                               const float* background_table, float* batch_rays, float* batch_rays_torso, float* target_s,
                               float* bc_rgb, void* stream);

/*
 * Frame scores: how far a rendered frame is from its ground truth, on the device.  Additive entries: the ABI version is unchanged.
 *
 * pred [H, W, 3] fp32, truth [H, W, 3] uint8, regions [H, W] uint8 (the region byte map idealnerf_sample_pixels draws from: bit 0
 * rect, 1 outside, 2 mouth, 3 torso) or NULL -> out [5, 4] float64.  Row 0 is the whole frame, rows 1..4 the pixels carrying bit
 * 0..3 of the region byte (zero rows with regions == NULL).  Columns:
 *   0 n_pixels   pixels of the group
 *   1 sse        sum over those pixels and the 3 channels of (pred - t)^2 with t = float(truth) / 255.0f: the reference's
 *                img2mse(rgb, target) times its element count (NeRFs/HeadNeRF/helper.py:150; target = uint8 / 255,
 *                train/audio_exp_nerf.py:126), so that PSNR = mse2psnr(sse / (3 n_pixels)) = -10 log10(mse) (helper.py:151).
 *                Difference and square in fp32, as the reference's; accumulation in fp64.
 *   2 n_windows  SSIM windows whose CENTRE pixel is in the group
 *   3 ssim_sum   sum over those windows and the 3 channels of the SSIM index (Wang et al. 2004): 11 x 11 Gaussian window, sigma
 *                1.5, separable, its 11 weights normalised in fp64 and rounded to fp32; "valid" windows only, (H - 10) x (W - 10)
 *                centres; data range 1, C1 = 1e-4, C2 = 9e-4; weighted biased variances E[x^2] - mu^2.  The window sums and the
 *                index are evaluated in fp64 (E[x^2] - mu^2 cancels against C2: fp32 sums move a window by 3e-4).
 *                H < 11 or W < 11: columns 2 and 3 are zero.
 * Deterministic: per-workgroup partial sums in the workspace, added in index order by a final pass, no floating-point atomics --
 * the same inputs give the same 160 bytes.  Nothing is read back to the host.  workspace:
 * idealnerf_frame_scores_workspace_bytes(H, W) bytes (20 doubles per IDN_SCORE_TILE^2 tile of the frame), 8-byte aligned.
 * H <= 0, W <= 0, a NULL pred / truth / out or a short workspace return IDN_EINVAL before any launch.
 */
#define IDN_SCORE_TILE 32 /* edge of the pixel tile one workgroup scores */
size_t idealnerf_frame_scores_workspace_bytes(int H, int W);
int idealnerf_frame_scores(const float* pred, const uint8_t* truth, const uint8_t* regions, int H, int W, double* out,
                           void* workspace, size_t workspace_bytes, void* stream);

/*
 * SSIM as a training loss, on contiguous patches of a ray batch.  Additive entries: the ABI version is unchanged.
 *
 * idealnerf_patch_pixels: sel_out receives the n_patches * p * p flat row-major pixel indices (y * W + x) of the p x p patches
 * whose top-left corners are (oy[k], ox[k]): patch by patch, row-major inside a patch -- the rows a [n_patches, p, p, 3] tensor
 * has.  The set travels by value as kernel arguments, as cameras do.  n_patches outside 1..IDN_PATCH_MAX, p outside
 * IDN_PATCH_MIN_P..IDN_PATCH_MAX_P, a negative origin, ox[k] + p > W, W <= 0 or a NULL pointer return IDN_EINVAL before any launch.
 * (The frame's height is the caller's: idealnerf_gather_rays turns indices past the frame into zero rows.)
 *
 * idealnerf_ssim_patch_fwd: pred, truth [n_patches, p, p, 3] fp32 -> out [n_patches + 1] float64: out[k] is patch k's mean SSIM
 * index over its 3 (p - 10)^2 windows (three channels, "valid" windows), out[n_patches] = 1 - mean(out[0 .. n_patches)), the
 * loss.  The index is idealnerf_frame_scores': the same eleven fp32 weights widened to fp64, C1 = 1e-4, C2 = 9e-4, weighted
 * biased variances, all five window moments and the index in fp64.
 *
 * idealnerf_ssim_patch_bwd: d_pred [n_patches, p, p, 3] fp32 is OVERWRITTEN with g * d loss / d pred, rounded once to fp32.  With
 * the window's moments mu_x, mu_t, E[xx], E[tt], E[xt] recomputed as the forward computes them and A = dS / d mu_x,
 * B = dS / d E[xx], C = dS / d E[xt] per window, every pixel gathers from the at most 121 windows that cover it:
 *     d_pred = -((g / n_patches) / (3 (p - 10)^2)) (sum w A + 2 x sum w B + t sum w C),   w = the pixel's weight in the window.
 * truth gets no gradient.
 *
 * Both: arithmetic beyond the loads is fp64; no floating-point atomics; every sum runs in a fixed order (a lane's items in index
 * order, a fixed shuffle tree, waves and patches in index order): the same inputs give the same bytes, and a patch's result
 * does not depend on the other patches of the call.  Limits and NULL pointers as idealnerf_patch_pixels: IDN_EINVAL.
 */
#define IDN_PATCH_MAX 16   /* patches of one set */
#define IDN_PATCH_MIN_P 11 /* one SSIM window */
#define IDN_PATCH_MAX_P 48 /* what one workgroup's 64 KiB of LDS hold: two fp32 tiles and three fp64 planes of 38^2 */
typedef struct idn_patch_set {
    int n_patches;
    int p;                 /* edge of every patch */
    int oy[IDN_PATCH_MAX]; /* top-left corners: row, */
    int ox[IDN_PATCH_MAX]; /* column */
} idn_patch_set;
int idealnerf_patch_pixels(const idn_patch_set* set, int W, int64_t* sel_out, void* stream);
int idealnerf_ssim_patch_fwd(const float* pred, const float* truth, int n_patches, int p, double* out, void* stream);
int idealnerf_ssim_patch_bwd(const float* pred, const float* truth, int n_patches, int p, float g, float* d_pred, void* stream);

size_t idealnerf_render_workspace_bytes(int64_t n_rays, int n_samples, int n_importance);
int idealnerf_render_rays_fwd(const idn_render_args* a, void* stream);

/*
 * Full-frame mode: Network.render_dynamic_face with `render_poses` (audio_exp_nerf.py:396-427) -- get_rays
 * (NeRFs/HeadNeRF/helper.py:228-243; the principal point defaults to W/2, H/2 as at :402), the viewing directions and the
 * [o, d, near, far, viewdir] records (:407-427) followed by batchify_rays / render_rays -- as ONE call: the rays of the pixels
 * [row0 * W, (row0 + nrows) * W) are derived on the device from the camera, one internal pass (32 768 rays) at a time into a
 * 1.4 MB scratch that stays L2-resident; no [H * W, 11] ray tensor exists and nothing is scattered to a rank but its
 * (row0, nrows).  `a->rays` must be NULL, `a->n_rays` = nrows * W, `a->bc_rgb` the band's background pixels; everything else as
 * idealnerf_render_rays_fwd (same kernels: the records are the ones idealnerf_frame_rays writes, bit for bit).
 * `rays_out` (may be NULL): [n_rays, 11] copy of the records (debug tap).
 */
typedef struct idn_frame {
    float c2w[12];        /* row-major [3][4] camera-to-world */
    int H, W;
    float focal, cx, cy;  /* cx, cy < 0: W/2, H/2 */
    float near_, far_;
    int row0, nrows;
    float* rays_out;
} idn_frame;
size_t idealnerf_render_frame_workspace_bytes(int64_t n_rays, int n_samples, int n_importance);
int idealnerf_render_frame_fwd(const idn_render_args* a, const idn_frame* frame, void* stream);

/*
 * The two render entries with options.  Additive entries: idn_render_args and the ABI version are unchanged, and the
 * entries above are these with opts == NULL (the defaults).
 *
 * colour_gate (default 1): the fp32 kernel sequence (fused_march == 0) launches its coarse and fine network kernels in a
 * form that skips the colour branch (views_linears.*, rgb_linear: 12.4 % of a pass) for every 128-point tile in which NO
 * point's colour can reach a pixel, and writes the raw colour 0.0f for it.  A point's colour cannot when the point is the
 * last sample of its ray (raw2outputs replaces its colour by the background pixel), or when its sigma <= 0 and its
 * spacing |z[s+1] - z[s]| * |rays_d| <= idealnerf_colour_gate_max_dist(): then alpha = 1 - expf(-1e-6 * dist) is exactly 0,
 * so is the weight, and weight * colour is +0 whatever the colour.  Sigma is computed as ever.  Every output of the render
 * is bit-identical to the ungated run; the one exception is a zero-weight sample whose colour branch ALONE overflows to
 * NaN / inf while its sigma is finite and <= 0 -- ungated that NaN reaches the pixel as 0 * NaN, gated it does not.
 * The gate is off (the ungated kernel is launched) for a pass whose density noise (noise_coarse / noise_fine) or raw tap
 * (tap_raw_coarse / tap_raw_fine) is given, for every arithmetic but IDN_PREC_F32, and in the fused arrangements.
 * gate_counters (may be NULL): device int64 [2][2] = (coarse, fine) x (tiles, skipped); the gated launches ADD their tile
 * counts to it (the caller zeroes it); a pass that ran ungated adds nothing.
 */
typedef struct idn_render_opts {
    int colour_gate;        /* 1 default, 0 off */
    int64_t* gate_counters; /* device, [2][2], or NULL */
} idn_render_opts;
int idealnerf_render_rays_fwd_opts(const idn_render_args* a, const idn_render_opts* opts, void* stream);
int idealnerf_render_frame_fwd_opts(const idn_render_args* a, const idn_frame* frame, const idn_render_opts* opts, void* stream);
float idealnerf_colour_gate_max_dist(void);

/* ------------------------------------------------------------------------------------------
 * Training step (NeRFs/HeadNeRF/train/audio_exp_nerf.py:534-552).  The forward of a pass is
 * idealnerf_coarse_depths / _query_rays_train_fwd / _composite_fwd / _sample_pdf_fwd; the
 * backward of a pass is one call.  z_samples are detached upstream (:345), so depths carry
 * no gradient; gradients reach the network parameters and the per-frame aud / latent vectors.
 * ------------------------------------------------------------------------------------------ */

/* Floats of the activation slab idealnerf_query_rays_train_fwd fills for n_points points
 * (2560 columns of saved activations + 88 floats of packed ReLU masks, x n_points rounded up to 128 rows;
 * need not be initialised). */
size_t idealnerf_train_acts_floats(int64_t n_points);

/* idealnerf_query_rays_fwd that also records what the backward needs (the post-ReLU
 * activations of all 11 hidden layers and both encodings).  precision: IDN_PREC_F32 or IDN_PREC_BF16X6 (the
 * fp32-grade arithmetics; `packed` must be that precision's stream).  idealnerf_pass_bwd itself computes the delta
 * chain and the 256 x 256 weight-gradient products with the six-piece bf16 arithmetic, or on
 * the fp32 matrix pipe when the process was started with IDN_BACKWARD_PIPE=f32. */
int idealnerf_query_rays_train_fwd(const float* packed, const float* folded, int precision, const float* rays,
                                   const float* z, int64_t n_rays, int n_samples, float* raw, float* acts,
                                   void* stream);
/* The same for a network of pts_ch / views_ch input columns (3 + 6 multires each, as idealnerf_facenerf_fwd_ch takes them):
 * the slab's x0 / dir matrices hold the network's own columns and zeros beyond them, as idealnerf_facenerf_train_fwd_ch
 * leaves them.  raw is the same either way (the stream holds zeros in those columns); the entry above is this one at 63 / 27. */
int idealnerf_query_rays_train_fwd_ch(const float* packed, const float* folded, int precision, const float* rays,
                                      const float* z, int64_t n_rays, int n_samples, int pts_ch, int views_ch, float* raw,
                                      float* acts, void* stream);

/* Gradient tensors, same shapes/layout as idn_facenerf_params (every entry is overwritten,
 * including the conditioning columns). */
typedef struct idn_facenerf_grads {
    float* pts_w[8];
    float* pts_b[8];
    float* views_w[3];
    float* views_b[3];
    float* alpha_w;
    float* alpha_b;
    float* rgb_w;
    float* rgb_b;
} idn_facenerf_grads;

size_t idealnerf_pass_bwd_workspace_bytes(int64_t n_rays, int n_samples);

/*
 * Backward of raw2outputs + run_network + FaceNeRF for one pass of n_rays x n_samples points.
 *   g_rgb_map [n,3], g_rgb_fg [n,3], g_last_weight [n], g_acc [n]: upstream gradients of the
 *   compositing outputs (any may be NULL = zero).
 *   d_aud [dim_aud], d_latent [dim_latent]: ACCUMULATED (+=); may be NULL.
 */
int idealnerf_pass_bwd(const idn_facenerf_params* p, const idn_facenerf_grads* grads, const float* aud,
                       const float* expr, const float* latent, const float* acts, const float* raw, const float* z,
                       const float* rays, const float* bc_rgb, int64_t n_rays, int n_samples, const float* g_rgb_map,
                       const float* g_rgb_fg, const float* g_last_weight, const float* g_acc, float* d_aud,
                       float* d_latent, void* workspace, size_t workspace_bytes, void* stream);

/*
 * idealnerf_pass_bwd that also returns the gradient of the pass's ray records (joint camera-pose refinement): the
 * arguments of idealnerf_pass_bwd plus d_rays [n_rays, IDN_RAY_FLOATS], OVERWRITTEN, in the layout of the record --
 * columns 0:3 d rays_o, 3:6 d rays_d, 8:11 d viewdirs, columns 6 and 7 (near, far) are written as 0.  It runs the same
 * backward (every other output is bit for bit idealnerf_pass_bwd's), then the input-row gradient of the pass's points
 * (into the workspace: the size idealnerf_pass_bwd_workspace_bytes names is enough) and its reduction per ray:
 *   encoding backward (helper.py:174-224, audio_exp_nerf.py:331,380): d pts[a] = dx[a] + sum_k 2^k (cos(2^k p_a) dx_sin[k, a]
 *     - sin(2^k p_a) dx_cos[k, a]) over the network's multires bands (10 by default), the same over its multires_views bands
 *     (4) for the view direction -- with no band, d pts = dx; points recomputed from rays and z as the forward does;  d rays_o = sum_s d pts_s, d rays_d = sum_s z_s d pts_s, d viewdirs = sum_s d dir_s;
 *   raw2outputs' dists = dz * |rays_d| (baseline.py:341-343): d rays_d += (sum_{s < S-1} dL/d dist_s dz_s) rays_d / |rays_d|
 *     (the last sample's 1e10 spacing saturates alpha and is left out).
 * Depths carry no gradient (coarse depths depend on near / far alone; fine depths are detached upstream, :345); the
 * background, the expression and near / far get none here (the first two: idealnerf_pass_bwd_ex).  Fixed summation order, no float atomics: a ray's gradient is a
 * function of the inputs alone, wherever the ray stands in the batch.  d_rays == NULL: exactly idealnerf_pass_bwd.
 * Argument errors return IDN_EINVAL, a short workspace IDN_EWORKSPACE, before any HIP call.  The frozen plan
 * (idealnerf_pass_bwd_cond) has no such variant.  Additive entry: the ABI version is unchanged.
 */
int idealnerf_pass_bwd_rays(const idn_facenerf_params* p, const idn_facenerf_grads* grads, const float* aud,
                            const float* expr, const float* latent, const float* acts, const float* raw, const float* z,
                            const float* rays, const float* bc_rgb, int64_t n_rays, int n_samples, const float* g_rgb_map,
                            const float* g_rgb_fg, const float* g_last_weight, const float* g_acc, float* d_aud,
                            float* d_latent, float* d_rays, void* workspace, size_t workspace_bytes, void* stream);

/*
 * idealnerf_pass_bwd for a FROZEN network (the head pair of the torso stage, train_torso.py:476-479): none of its parameters
 * takes a gradient, but the conditioning it was given does.  The arguments of idealnerf_pass_bwd without `grads`, the same
 * workspace size; d_aud / d_latent are ACCUMULATED (+=) exactly as idealnerf_pass_bwd documents, and nothing else is written.
 * It runs that entry's compositing backward and delta chain, then -- instead of the sixteen weight-gradient products -- the
 * column sums of the two delta matrices the conditioning reaches (pts_linears.0 and .5; fp64, fixed order, no atomics: the
 * result is a function of the inputs alone) and the conditioning range of the fold.  Both d_aud and d_latent NULL: nothing
 * is launched.  Additive entry: the ABI version is unchanged.
 */
int idealnerf_pass_bwd_cond(const idn_facenerf_params* p, const float* aud, const float* expr, const float* latent,
                            const float* acts, const float* raw, const float* z, const float* rays, const float* bc_rgb,
                            int64_t n_rays, int n_samples, const float* g_rgb_map, const float* g_rgb_fg,
                            const float* g_last_weight, const float* g_acc, float* d_aud, float* d_latent, void* workspace,
                            size_t workspace_bytes, void* stream);

/*
 * Optional outputs of idealnerf_pass_bwd_ex; every field may be NULL, and a NULL struct pointer is a struct of NULLs.
 *   d_expr [dim_expr]: ACCUMULATED (+=), like d_aud:
 *     d expr[e] = (d cond[dim_aud + e] + sum_n Wv0[n][256 + views_ch + e] dbv'[n]) / 3
 *     (expr / 3 enters pts_linears.0, pts_linears.5 and views_linears.0, face_nerf.py:49; dbv' is views_linears.0's bias
 *     gradient).  The expression's weight-gradient columns are what they were.  Non-NULL for a network with dim_expr == 0
 *     (or with expr == NULL): IDN_EINVAL.
 *   d_rays [n_rays, IDN_RAY_FLOATS]: OVERWRITTEN, exactly as idealnerf_pass_bwd_rays documents.
 *   d_views0_bias [128]: OVERWRITTEN; the frozen plan only (with grads it is grads->views_b[0]: IDN_EINVAL).  The gradient of
 *     views_linears.0's bias, for a caller whose conditioning also reaches that bias; it needs one of d_aud / d_latent /
 *     d_expr (IDN_EINVAL otherwise: with none of them the pass is not run).
 */
typedef struct idn_pass_bwd_extra {
    float* d_expr;
    float* d_rays;
    float* d_views0_bias;
} idn_pass_bwd_extra;

/*
 * The pass backward with every optional gradient: the arguments of idealnerf_pass_bwd plus `extra`.
 *   grads != NULL: the training plan.  With d_expr the conditioning fold also sums the expression's columns of
 *     views_linears.0 against that layer's bias gradient; with d_rays the entry is idealnerf_pass_bwd_rays.
 *   grads == NULL: the frozen plan, idealnerf_pass_bwd_cond.  d_expr / d_views0_bias need dbv' there: the column sums, over
 *     the pass's n_rays * n_samples points (never the padding rows up to a multiple of 128), of the views_linears.0 deltas
 *     the delta chain leaves in the workspace -- summed as that entry sums pts_linears.0 / .5: fp64, row blocks in row order,
 *     partial sums added in block order, no atomics.  It runs when any of d_aud, d_latent, d_expr is wanted and launches
 *     nothing when none is.  d_rays there: IDN_EUNSUPPORTED.
 * Every output the three entries above share is bit for bit theirs, whatever `extra` asks for; with every extra NULL the
 * entry IS the corresponding one of them (they call the same host function).  The background takes no kernel:
 * rgb_map is linear in bc_rgb with the pass's last_weight as coefficient, d bc = g_rgb_map * last_weight[:, None].  Near /
 * far and depths still get no gradient.  Argument errors return before any HIP call.  Additive entry: the ABI version is
 * unchanged.
 */
int idealnerf_pass_bwd_ex(const idn_facenerf_params* p, const idn_facenerf_grads* grads, const float* aud,
                          const float* expr, const float* latent, const float* acts, const float* raw, const float* z,
                          const float* rays, const float* bc_rgb, int64_t n_rays, int n_samples, const float* g_rgb_map,
                          const float* g_rgb_fg, const float* g_last_weight, const float* g_acc, float* d_aud,
                          float* d_latent, const idn_pass_bwd_extra* extra, void* workspace, size_t workspace_bytes,
                          void* stream);

/*
 * FaceNeRF.forward with gradients (models/face_nerf.py:40-80): the module trained on pre-embedded rows, outside
 * render_rays -- weights, input rows and conditioning vectors.
 *
 * idealnerf_facenerf_train_fwd (models/face_nerf.py:40-80): idealnerf_facenerf_fwd that also records what the backward
 *   needs.  precision: IDN_PREC_F32 or IDN_PREC_BF16X6 (`packed` is that precision's stream).  acts: idealnerf_train_acts_floats(n)
 *   floats, the slab layout of idealnerf_query_rays_train_fwd; its x0 / dir matrices hold x[:, 0:63] / x[:, 63:90] (zero-padded
 *   to 64 columns), and every padding row up to n rounded up to 128 is defined (it repeats the last row).
 *   out[n, 4] equals idealnerf_facenerf_fwd's at the same precision bit for bit: each saving kernel runs the arithmetic of
 *   its inference kernel (bias first, the same MFMA order, the same head dot products) plus the slab stores.
 */
int idealnerf_facenerf_train_fwd(const float* packed, const float* folded, int precision, const float* x, int64_t n,
                                 float* out, float* acts, void* stream);
/* The same for x[n, pts_ch + views_ch] (widths as idealnerf_facenerf_fwd_ch): the slab's x0 / dir matrices hold
 * x[:, 0:pts_ch] / x[:, pts_ch:], zero-padded to 64 columns.  The entry above is this one at 63 / 27. */
int idealnerf_facenerf_train_fwd_ch(const float* packed, const float* folded, int precision, const float* x, int pts_ch,
                                    int views_ch, int64_t n, float* out, float* acts, void* stream);

/* Workspace of idealnerf_facenerf_bwd for n rows (the size idealnerf_pass_bwd needs for n points). */
size_t idealnerf_facenerf_bwd_workspace_bytes(int64_t n);

/*
 * Backward of FaceNeRF.forward (models/face_nerf.py:40-80) for n rows, from the slab idealnerf_facenerf_train_fwd filled.
 *   g_out [n, 4]: dL / d out, in the (rgb_raw, sigma_raw) order of idealnerf_facenerf_fwd.
 *   grads: OVERWRITTEN, every entry including the conditioning columns (as idealnerf_pass_bwd); feature_linear has none.
 *   d_x [n, pts_ch + views_ch] (the widths `p` names; [n, 90] at the defaults): OVERWRITTEN with dL / dx; NULL skips its kernel.
 *   d_aud [dim_aud], d_expr [dim_expr], d_latent [dim_latent]: ACCUMULATED (+=); any may be NULL.  expr enters all three
 *   layers as expr * 1 / 3 (face_nerf.py:49): d_expr = (db0 . W0[:, expr] + db5 . W5[:, expr] + dbv0 . Wv0[:, expr]) / 3.
 * n == 0 writes nothing.  Argument errors return IDN_EINVAL before any launch; a short workspace IDN_EWORKSPACE.
 */
int idealnerf_facenerf_bwd(const idn_facenerf_params* p, const idn_facenerf_grads* grads, const float* aud, const float* expr,
                           const float* latent, const float* acts, int64_t n, const float* g_out, float* d_x, float* d_aud,
                           float* d_expr, float* d_latent, void* workspace, size_t workspace_bytes, void* stream);

/*
 * Test aid (no reference counterpart): one 256 x 256 weight-gradient product of the training step in isolation,
 *   dW[256][256] = delta[rows, :256]^T . acts[rows, :256],   db[256] = column sums of delta (may be NULL),
 * rows a positive multiple of 128, row pitches >= 256 floats.  pipe = IDN_DW_PIPE_BF16X6: as idealnerf_pass_bwd computes
 * the 256-wide layers (each fp32 operand as the exact sum of three bf16 pieces, six piece products per product on the bf16
 * matrix pipe, fp32 accumulate); IDN_DW_PIPE_F32: the same product on the fp32 matrix pipe.  tests/ compares both with fp64.
 */
#define IDN_DW_PIPE_BF16X6 0
#define IDN_DW_PIPE_F32 1
#define IDN_DW_PIPE_BF16X6_PASS 2   /* BF16X6 with the split count of a training pass (2 #CUs / 9 workgroups: each keeps its fp32
                                       accumulators over 1/56 of the rows on a 256-CU part), not one split per CU */
size_t idealnerf_dw_gemm_workspace_bytes(void);
int idealnerf_dw_gemm(const float* delta, int ld_delta, const float* acts, int ld_acts, int64_t rows, float* dW, float* db,
                      int pipe, void* workspace, size_t workspace_bytes, void* stream);

/*
 * Test aid (no reference counterpart): a LIST of weight-gradient products through one pass plan, as a training pass runs
 * them -- every shape the backward is built for (256 x 256, 128 x 128, 128 x 256, 256 x 64, 128 x 64, 64 x 128 as N x K), the
 * 256 x 256 ones of the bf16-piece pipe as one batched launch, every block taken out by the pass's one reduction launch.
 *   product i:  part = delta[rows, :N]^T . acts[rows, :K]  (acts2 != NULL, bf16-piece pipe, 256 x 256 only: output columns
 *               0..127 from acts[:, :128], columns 128..255 from acts2[:, :128], both at pitch ld_acts and less than
 *               2 GiB apart: one allocation, as the activation slab of a pass is);
 *   take:       out[r * ldo + c] = part[row0 + r][col0 + c], r < rows, c < cols -- nothing else of `out` is written;
 *   colsum take: out[c] = column sum of delta[:, col0 + c], c < cols (want_colsum must be set).
 * rows: a positive multiple of 128; pitches in floats, multiples of 4, >= N / K (ld_acts >= 128 with acts2); operand
 * pointers 16-byte aligned.
 * pipe: IDN_DW_PIPE_BF16X6 (the 256 x 256 products as bf16 pieces, x6_items = how many of them the list may name: the CUs
 * are divided among that many) or IDN_DW_PIPE_F32 (every product on the fp32 matrix pipe; x6_items is not used).
 * On success every record's `splits` / `chunks_per_split` hold the plan it ran with.  Argument errors are found before any
 * HIP call: IDN_EINVAL, IDN_EUNSUPPORTED (a shape with no kernel), IDN_EWORKSPACE.
 */
#define IDN_DW_MAX_PRODUCTS 16
#define IDN_DW_MAX_TAKES 4
#define IDN_DW_MAX_COLSUM_TAKES 2
typedef struct idn_dw_take {
    int row0, col0, rows, cols;
    float* out;
    int ldo;
} idn_dw_take;
typedef struct idn_dw_colsum_take {
    int col0, cols;
    float* out;
} idn_dw_colsum_take;
typedef struct idn_dw_product {
    const float* delta;
    int ld_delta, N;
    const float* acts;
    int ld_acts, K;
    const float* acts2;
    int want_colsum;
    int n_takes;
    idn_dw_take takes[IDN_DW_MAX_TAKES];
    int n_colsum_takes;
    idn_dw_colsum_take colsum_takes[IDN_DW_MAX_COLSUM_TAKES];
    int splits, chunks_per_split; /* out */
} idn_dw_product;
size_t idealnerf_dw_products_workspace_bytes(void);
int idealnerf_dw_products(int64_t rows, int pipe, int x6_items, idn_dw_product* products, int n, void* workspace,
                          size_t workspace_bytes, void* stream);

/*
 * Test aid (no reference counterpart): the backward delta chain of a training pass alone -- the transposed-weight pack and
 * the fused chain kernel, exactly the two launches idealnerf_pass_bwd / idealnerf_facenerf_bwd make between the head deltas
 * and the weight-gradient products -- on the caller's matrices, so that tests/ can hold every element of the eleven delta
 * matrices to fp64.
 *   pipe:   IDN_DW_PIPE_BF16X6 (what a pass runs) or IDN_DW_PIPE_F32 (what it runs under IDN_BACKWARD_PIPE=f32).
 *   acts:   a slab of idealnerf_train_acts_floats(p_pad) floats; only its ReLU-mask tail is read.
 *   d_rgb:  [p_pad, 64], columns 0..2 = d raw rgb; the other columns are not read.
 *   dv0:    [p_pad, 256], in and out: column 128 = d raw sigma on entry; columns 0..127 are WRITTEN with views_linears.0's
 *           delta; columns 129..255 are neither read nor written.
 *   dv21:   [p_pad, 256], WRITTEN: views_linears.2's delta in columns 0..127, views_linears.1's in columns 128..255.
 *   da:     [8][p_pad, 256], WRITTEN: da[l] = delta of pts_linears.l.
 *   max_blocks: 0 = the grid of a pass, min(p_pad / 128, CUs); k > 0 caps it at k workgroups, so that a call of a few
 *           hundred rows makes one workgroup walk several 128-row tiles.  blocks_out (may be NULL): the grid that ran.
 *   workspace: idealnerf_delta_chain_workspace_bytes() bytes, the transposed weight stream.
 * p_pad: a positive multiple of 128, at most 2^24; every pointer 16-byte aligned.  Argument errors are found before any
 * HIP call: IDN_EINVAL, IDN_EUNSUPPORTED (p_pad above 2^24), IDN_EWORKSPACE.  Additive entry: the ABI version is unchanged.
 */
size_t idealnerf_delta_chain_workspace_bytes(void);
int idealnerf_delta_chain(const idn_facenerf_params* p, int pipe, const float* acts, int64_t p_pad, const float* d_rgb,
                          float* dv0, float* dv21, float* da, int max_blocks, int* blocks_out, void* workspace,
                          size_t workspace_bytes, void* stream);

/*
 * Test aid (no reference counterpart): the compositing backward of a training pass alone -- the first launch of
 * idealnerf_pass_bwd*, through the same dispatch (one kernel per ceil(n_samples / 64) = 1..8, each with and without the
 * |rays_d| gradient) -- so that tests/ can hold every element of d raw to fp64.
 *   raw [n_rays, n_samples, 4] (16-byte aligned), z [n_rays, n_samples], rays [n_rays, 11], bc_rgb [n_rays, 3]: as idealnerf_pass_bwd.
 *   g_rgb_map [n_rays, 3], g_rgb_fg [n_rays, 3], g_last_weight [n_rays], g_acc [n_rays]: dL / d output; each may be NULL (= zeros).
 *   d_rgb, ld_rgb: WRITTEN, d raw rgb of point p = ray * n_samples + s at d_rgb[p * ld_rgb + 0..2] (ld_rgb >= 3);
 *   d_sig, ld_sig: WRITTEN, d raw sigma of point p at d_sig[p * ld_sig] (ld_sig >= 1).  A pass runs ld_rgb = 64 and ld_sig = 256,
 *           d_sig at column 128 of its [p_pad, 256] delta matrix; (4, 4) with d_sig = d_rgb + 3 fills one [n_rays, n_samples, 4] tensor.
 *   d_norm, ld_norm: NULL, or WRITTEN with dL / d |rays_d| of ray r at d_norm[r * ld_norm] (a pass: column 6 of d_rays, pitch 11).
 *           d_rgb and d_sig are the same bits either way.
 * Nothing else is written.  n_rays == 0 writes nothing.  Argument errors are found before any HIP call: IDN_EINVAL (a NULL
 * operand, a pitch below 3 / 1 / 1, raw unaligned), IDN_EUNSUPPORTED (n_samples outside [2, 512]).  Additive entry: the ABI version is unchanged.
 */
int idealnerf_composite_bwd(const float* raw, const float* z, const float* rays, const float* bc_rgb, int64_t n_rays,
                            int n_samples, const float* g_rgb_map, const float* g_rgb_fg, const float* g_last_weight,
                            const float* g_acc, float* d_rgb, int ld_rgb, float* d_sig, int ld_sig, float* d_norm, int ld_norm,
                            void* stream);

/*
 * Test aids (no reference counterpart): what a training backward runs after the delta chain, stage by stage, on the caller's
 * matrices -- the same kernels through the same launch functions as idealnerf_pass_bwd* / idealnerf_facenerf_bwd -- so that
 * tests/ can hold every element to fp64.  Argument errors are found before any HIP call.  Additive entries: the ABI version
 * is unchanged.
 *
 * idealnerf_input_grad: the input-row gradient alone.  dA0 / dA5 / dV0 [p_pad, 256] (16-byte aligned): the deltas of
 *   pts_linears.0, pts_linears.5 and views_linears.0 (dV0: columns 0..127; columns 128..255 are not read).  d_x
 *   [n, pts_ch + views_ch] of the network `p` describes is WRITTEN; nothing else is.  p_pad: a positive multiple of 128, at most
 *   2^24; 1 <= n <= p_pad.  Of the weights only pts_linears.0 / .5's encoding columns and views_linears.0's direction columns
 *   are read.  max_blocks: 0 = the grid of a pass, min(ceil(p_pad / 512), CUs); k > 0 caps it at k workgroups.  blocks_out
 *   (may be NULL): the grid that ran.
 * idealnerf_ray_grad: the encoding backward and the per-ray reduction alone.  d_x [n_rays * n_samples, pts_ch + views_ch],
 *   rays [n_rays, 11], z [n_rays, n_samples]; d_rays [n_rays, 11]: column 6 is READ (dL / d |rays_d|), columns 0..10 are WRITTEN
 *   (6 and 7 with zeros).  IDN_EINVAL for widths that are not 3 + 6 L, IDN_EUNSUPPORTED for n_samples outside [2, 512].
 * idealnerf_fold_bwd: the conditioning fold's backward alone.  db0 / db5 [256], dbv [128]: the bias gradients of pts_linears.0 / .5
 *   and views_linears.0.  With gW0, gW5, gWv0 (the three layers' gradient tensors in nn.Linear layout) their conditioning
 *   columns are WRITTEN; with all three NULL the launch covers d cond alone, as the frozen plan of idealnerf_pass_bwd_ex
 *   (one or two NULL: IDN_EINVAL).  d_aud / d_expr / d_latent: ACCUMULATED, each may be NULL; dbv is read only for the
 *   expression columns of gWv0 and for d_expr.  A network without conditioning writes nothing.
 * idealnerf_cond_colsums: the column sums the frozen plan feeds that fold with.  db [2][256] = the sums of dA0 | dA5 over all
 *   p_pad rows; dbv [128] = the sums of dV0[:, 0:128] over the first P rows.  Either group (dA0, dA5, db) / (dV0, dbv) may be
 *   NULL as a whole.  workspace: idealnerf_cond_colsums_workspace_bytes() bytes, 8-byte aligned (IDN_EWORKSPACE).
 */
int idealnerf_input_grad(const idn_facenerf_params* p, const float* dA0, const float* dA5, const float* dV0, int64_t n,
                         int64_t p_pad, float* d_x, int max_blocks, int* blocks_out, void* stream);
int idealnerf_ray_grad(const float* d_x, int pts_ch, int views_ch, const float* rays, const float* z, int64_t n_rays, int n_samples,
                       float* d_rays, void* stream);
int idealnerf_fold_bwd(const idn_facenerf_params* p, const float* aud, const float* expr, const float* latent, const float* db0,
                       const float* db5, const float* dbv, float* gW0, float* gW5, float* gWv0, float* d_aud, float* d_expr,
                       float* d_latent, void* stream);
size_t idealnerf_cond_colsums_workspace_bytes(void);
int idealnerf_cond_colsums(const float* dA0, const float* dA5, const float* dV0, int64_t P, int64_t p_pad, float* db, float* dbv,
                           void* workspace, size_t workspace_bytes, void* stream);

/*
 * AudioNet.forward (models/audio_net.py:43-69: the per-frame audio latent of audio_exp_nerf.py:258-259, or of the eight windows
 * under the attention smoother, :235-257) as ONE kernel, and its backward as one: windows [n, 16, 29] (win_size 16) ->
 * out [n, dim_aud].  Parameters in nn.Conv1d / nn.Linear layout ([C_out, C_in, 3] / [out, in], fp32, contiguous):
 * encoder_conv.{0,2,4,6} and encoder_fc1.{0,2}.  `saved` (NULL for inference) receives the 640 post-activations per window the
 * backward needs (idealnerf_audio_net_saved_floats).  The backward (n <= 8 windows) OVERWRITES every gradient buffer with the
 * sum over the windows; the windows themselves are data (no gradient).
 */
typedef struct idn_audio_net_params {
    const float* conv_w[4];
    const float* conv_b[4];
    const float* fc_w[2];
    const float* fc_b[2];
    int dim_aud;
} idn_audio_net_params;
typedef struct idn_audio_net_grads {
    float* conv_w[4];
    float* conv_b[4];
    float* fc_w[2];
    float* fc_b[2];
} idn_audio_net_grads;
size_t idealnerf_audio_net_saved_floats(int n_windows);
int idealnerf_audio_net_fwd(const idn_audio_net_params* p, const float* windows, int n_windows, float* out, float* saved,
                            void* stream);
int idealnerf_audio_net_bwd(const idn_audio_net_params* p, const idn_audio_net_grads* grads, const float* windows,
                            const float* saved, const float* d_out, int n_windows, void* stream);

/*
 * Frame tail.  to8b = `(255 * np.clip(x, 0, 1)).astype(np.uint8)` (NeRFs/HeadNeRF/helper.py:154) on
 * the device: rgb [n_pixels,3] fp32 -> out [n_pixels,3] u8, bit-identical to numpy for finite input;
 * swap_rb != 0 writes the channels in reverse order (the cv2.cvtColor the reference leaves
 * commented out, test/eval_aud_exp_nerf.py:490).  nonfinite_flag (device int, may be NULL) is
 * OR-ed with 1 if any input value is NaN/Inf: one flag per frame replaces the reference's
 * per-chunk isnan/isinf host syncs (train/audio_exp_nerf.py:367-369); such a value is written as 0.
 */
int idealnerf_to8b(const float* rgb, int64_t n_pixels, int swap_rb, uint8_t* out, int* nonfinite_flag, void* stream);

/* Tail of the head + torso clip loop (NeRFs/TorsoNeRF/test_torso.py:523-525, train_torso.py:269-270) as one kernel:
 *   out = to8b(rgb_head * last_weight[:, None] + rgb_fg)
 * rgb_head [n,3], last_weight [n], rgb_fg [n,3] fp32 -> out [n,3] u8; swap_rb and nonfinite_flag as idealnerf_to8b.
 * The product and the sum round once each (no contraction), so for a finite composite out equals idealnerf_to8b of the
 * eager expression bit for bit.  A NaN/Inf in any input makes the composite NaN/Inf: that value is written as 0 and
 * flagged (idealnerf_to8b writes 255 for +Inf, numpy's clip; both flag it).
 * fg_out (may be NULL): [n,3] u8 = idealnerf_to8b(rgb_fg), the every-10th-frame "_torso.jpg" still (test_torso.py:529-530).
 * Pointers that are 16-byte (inputs) / 4-byte (outputs) aligned take the four-pixels-per-thread path; any others are legal. */
int idealnerf_compose_to8b(const float* rgb_head, const float* last_weight, const float* rgb_fg, int64_t n_pixels,
                           int swap_rb, uint8_t* out, uint8_t* fg_out, int* nonfinite_flag, void* stream);

/* ------------------------------------------------------------------------------------------
 * Ray cull of the inference frame path (no reference counterpart).  Additive entries: the ABI
 * version is unchanged.
 *
 * A ray all of whose samples have sigma_raw <= 0 renders to its background pixel exactly (alpha = 1 - expf(-1e-6 dist) is
 * 0.0f while dist <= idealnerf_colour_gate_max_dist(); the last sample's alpha is 1 and its colour is the background).  An
 * occupancy grid built from the networks' own sigma lets such rays be recognised before any network is evaluated.
 *
 * Grid: G^3 cubic cells of edge `cell` over the box lo + [0, G cell]^3, G a multiple of 32 in 32..1024.
 *   corners  uint8 [(G+1)^3], index ((iz (G+1)) + iy) (G+1) + ix: lattice point lo + (ix, iy, iz) cell
 *   bits     uint32 [G^3 / 32], word (z G + y) (G / 32) + (x >> 5), bit x & 31: cell (x, y, z)
 */
/* corners[i] |= raw[i].w > sigma_min for i < n (raw [n, 4] = a network's output for lattice points; one thread per point). */
int idealnerf_cull_mark(const float* raw, int64_t n, float sigma_min, uint8_t* corners, void* stream);
/* A cell is occupied when any of its 8 corners is marked; the set is dilated by `dilate` >= 0 cells in Chebyshev distance
 * (clamped to G).  One thread computes one word of `bits`; every word is written. */
int idealnerf_cull_cells(const uint8_t* corners, int G, int dilate, uint32_t* bits, void* stream);

typedef struct idn_cull_grid {
    const uint32_t* bits; /* device, [G^3 / 32] */
    int G;
    float lo[3];
    float cell;
} idn_cull_grid;
/* classify + compact the pixels of the frame's row band.  Pixel q (row-major in the band) has the ray idealnerf_frame_rays
 * derives for it (the same device function); it is marched at z_k = near + k dz, k = 0..K-1, and z_K = far, and is LIVE when a
 * march point lies in an occupied cell or outside the box.  The caller chooses dz so that dz |d| <= cell / 2 for every ray of
 * the frame.  sel [nrows W] int64: the live pixels in ascending order in its first *n_live entries (the rest is not
 * written); n_live: device int32.  Count per workgroup, scan in index order, write: no atomics, the same bytes on every
 * run.  frame->rays_out is not read. */
size_t idealnerf_cull_classify_workspace_bytes(int64_t n_pixels);
int idealnerf_cull_classify(const idn_cull_grid* grid, const idn_frame* frame, float dz, int K, int64_t* sel, int32_t* n_live,
                            void* workspace, size_t workspace_bytes, void* stream);
/* rays [n, 11] and bc_live [n, 3] of the band's pixels sel[0..n): each row of rays is the row idealnerf_frame_rays writes for
 * that pixel, bit for bit; bc [nrows W, 3] is the band's background. */
int idealnerf_cull_gather(const int64_t* sel, int64_t n, const idn_frame* frame, const float* bc, float* rays, float* bc_live,
                          void* stream);
/* fill + scatter, for up to IDN_CULL_MAX_OUTPUTS outputs at once: dense [n_pixels, channels] receives the culled value in
 * every pixel (`value`, or with fill_background != 0 and channels == 3 the pixel of bc [n_pixels, 3]) and then row i of
 * live [n_live, channels] at pixel sel[i].  n_live == 0: the fill alone (live may be NULL). */
#define IDN_CULL_MAX_OUTPUTS 12
typedef struct idn_cull_output {
    float* dense;
    const float* live;
    int channels;        /* 1 or 3 */
    int fill_background; /* 0: `value`; 1: the background pixel */
    float value;
} idn_cull_output;
int idealnerf_cull_scatter(const int64_t* sel, int64_t n_live, int64_t n_pixels, const float* bc, const idn_cull_output* outputs,
                           int n_outputs, void* stream);

/* Sample cull of the live rays: a network pass over rays [n, 11] / z [n, S] evaluated only where
 * raw2outputs could tell the result from raw = (0, 0, 0, 0).  Point P = ray S + s lies at p = o + d z (product and sum
 * rounded separately, the network kernels' own point) and is SKIPPABLE when p lies inside the grid's box in a cell whose bit
 * is clear, and it is its ray's last sample (s == S - 1) or |dist| <= idealnerf_colour_gate_max_dist(), with
 * dist = (z[s + 1] - z[s]) sqrtf((dx dx + dy dy) + dz dz) as the compositing forms it.  Every other point is LIVE (occupied
 * cell, outside the box, wider spacing, a NaN anywhere).  Under the grid's contract (sigma_raw <= 0 in clear cells) the
 * compositing of the scattered raw has the bits of the compositing of the full network pass.
 * classify: sel [n S] int64 receives the live points in ascending order in its first *n_live entries (device int32; the
 * rest is not written); n S < 2^31; workspace: idealnerf_cull_classify_workspace_bytes(n S).  No atomics.
 * gather: pts [m, 3] / dirs [m, 3] of the points sel[0..m): idealnerf_query_points_fwd's inputs with n_samples = 1.
 * scatter: raw [n_points, 4] = +0.0f everywhere, then row j of raw_live [m, 4] at point sel[j] (each point at most once:
 * the same bytes on every run); both 16-byte aligned. */
int idealnerf_cull_sample_classify(const idn_cull_grid* grid, const float* rays, const float* z, int64_t n, int S, int64_t* sel,
                                   int32_t* n_live, void* workspace, size_t workspace_bytes, void* stream);
int idealnerf_cull_sample_gather(const int64_t* sel, int64_t m, const float* rays, const float* z, int64_t n, int S, float* pts,
                                 float* dirs, void* stream);
int idealnerf_cull_sample_scatter(const int64_t* sel, int64_t m, const float* raw_live, int64_t n_points, float* raw, void* stream);

/*
 * Measurement aid (no reference counterpart): between begin and end, every launch of
 * the fused PE+MLP kernel is bracketed by HIP events on its own stream.  end()
 * synchronises those events and returns the summed kernel time, the number of launches
 * and the number of points (ray-samples) they evaluated.  Process-wide; not for
 * concurrent use.
 */
void idealnerf_profile_begin(void);
int idealnerf_profile_end(double* total_ms, int64_t* launches, int64_t* points);

/* The same measurement split by kernel family (arrays of IDN_PROF_KINDS entries each; any may be NULL):
 * the training step's roofline needs its three MFMA kernels separately.  For the dW GEMMs `points` counts
 * the points each launch contracted over (one launch per layer). */
#define IDN_PROF_MLP_FWD 0      /* fused PE + MLP forward (inference) */
#define IDN_PROF_MLP_FWD_SAVE 1 /* the same with saved activations (training forward) */
#define IDN_PROF_DELTA_CHAIN 2  /* fused backward delta chain */
#define IDN_PROF_DW_GEMM 3      /* dW = delta^T . activation GEMMs (+ bias column sums) on the fp32 matrix pipe */
#define IDN_PROF_DW_GEMM_X6 4   /* the 256 x 256 dW GEMMs: six bf16 piece products per fp32 product, fp32 accumulate */
#define IDN_PROF_MLP_FWD_SAVE_X6 5 /* training forward as six bf16 piece products per fp32 product (IDN_PREC_BF16X6) */
#define IDN_PROF_DELTA_CHAIN_X6 6  /* backward delta chain, the same arithmetic */
#define IDN_PROF_KINDS 7
int idealnerf_profile_end_kinds(double* total_ms, int64_t* launches, int64_t* points);

#ifdef __cplusplus
}
#endif
#endif /* IDEALNERF_H */
