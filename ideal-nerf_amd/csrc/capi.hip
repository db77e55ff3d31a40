// extern "C" surface of libidealnerf.so (declared in include/idealnerf.h).
#include "idn_internal.h"
#include <cstdarg>
#include <cstdio>

namespace idn {

static thread_local char g_err[512] = "";

int fail(int code, const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
    return code;
}

static int check_precision(int precision) {
    if (precision == IDN_PREC_F32 || precision == IDN_PREC_BF16X3 || precision == IDN_PREC_BF16 || precision == IDN_PREC_FP16X3 ||
        precision == IDN_PREC_BF16X6)
        return IDN_OK;
    return fail(IDN_EUNSUPPORTED, "precision %d is unknown (IDN_PREC_F32, IDN_PREC_BF16X3, IDN_PREC_BF16, IDN_PREC_FP16X3, IDN_PREC_BF16X6)", precision);
}
static int check_precision_train(int precision) {
    if (precision == IDN_PREC_F32 || precision == IDN_PREC_BF16X6) return IDN_OK;
    return fail(IDN_EUNSUPPORTED, "the training path runs fp32-grade arithmetic only: IDN_PREC_F32 or IDN_PREC_BF16X6 (got %d)", precision);
}

int launch_mlp(int precision, const MlpArgs& a, hipStream_t s, MlpGate gate) {
    if (a.n_points > 0x7fffffffL) return fail(IDN_EUNSUPPORTED, "n_points %lld exceeds 2^31-1 per launch", (long long)a.n_points);
    if ((a.rays || a.pts) && a.S < 1) return fail(IDN_EINVAL, "n_samples < 1");
    if (precision == IDN_PREC_BF16X3) return launch_mlp_bf16x3(a, s);
    if (precision == IDN_PREC_BF16) return launch_mlp_bf16(a, s);
    if (precision == IDN_PREC_FP16X3) return launch_mlp_fp16x3(a, s);
    if (precision == IDN_PREC_BF16X6) return launch_mlp_bf16x6(a, s);
    return launch_mlp_f32(a, s, gate);
}

static int check_params(const idn_facenerf_params* p) {
    if (!p) return fail(IDN_EINVAL, "params is NULL");
    for (int i = 0; i < 8; ++i)
        if (!p->pts_w[i] || !p->pts_b[i]) return fail(IDN_EINVAL, "pts_linears.%d is NULL", i);
    for (int i = 0; i < 3; ++i)
        if (!p->views_w[i] || !p->views_b[i]) return fail(IDN_EINVAL, "views_linears.%d is NULL", i);
    if (!p->alpha_w || !p->alpha_b || !p->rgb_w || !p->rgb_b) return fail(IDN_EINVAL, "alpha/rgb head is NULL");
    if (p->dim_aud < 0 || p->dim_expr < 0 || p->dim_latent < 0) return fail(IDN_EINVAL, "negative conditioning width");
    // the encoding widths, stored as the value + 1 (0: the default 10 / 4)
    if (p->multires_plus1 < 0 || p->multires_plus1 > IDN_MAX_MULTIRES + 1)
        return fail(IDN_EINVAL, "multires_plus1 = %d: multires must be in 0..%d (0 in the field = the default %d)", p->multires_plus1,
                    IDN_MAX_MULTIRES, IDN_MAX_MULTIRES);
    if (p->multires_views_plus1 < 0 || p->multires_views_plus1 > IDN_MAX_MULTIRES_VIEWS + 1)
        return fail(IDN_EINVAL, "multires_views_plus1 = %d: multires_views must be in 0..%d (0 in the field = the default %d)",
                    p->multires_views_plus1, IDN_MAX_MULTIRES_VIEWS, IDN_MAX_MULTIRES_VIEWS);
    return IDN_OK;
}
// the row widths the x-mode entries are given: 3 + 6 L, L in 0..10 / 0..4
static int check_widths(int pts_ch, int views_ch) {
    if (pts_ch < 3 || pts_ch > IDN_PTS_CH || pts_ch % 6 != 3)
        return fail(IDN_EINVAL, "pts_ch %d is not 3 + 6 multires with multires in 0..%d (3..%d)", pts_ch, IDN_MAX_MULTIRES, IDN_PTS_CH);
    if (views_ch < 3 || views_ch > IDN_VIEWS_CH || views_ch % 6 != 3)
        return fail(IDN_EINVAL, "views_ch %d is not 3 + 6 multires_views with multires_views in 0..%d (3..%d)", views_ch,
                    IDN_MAX_MULTIRES_VIEWS, IDN_VIEWS_CH);
    return IDN_OK;
}

// ---- MLP launch timing (bench.py's roofline figure) ---------------------------------
// HIP events recorded on the launch stream itself, immediately around the kernel.
// Process-wide and meant for single-threaded measurement runs only.
static const int kProfSlots = 8192;
static bool g_prof_on = false;
static int g_prof_n = 0;
static hipEvent_t g_prof_ev[kProfSlots][2];
static int g_prof_created = 0;
static int64_t g_prof_points[kProfSlots];
static int g_prof_kind[kProfSlots];

ProfScope::ProfScope(hipStream_t s_, int64_t points, int kind) : slot(-1), s(s_) {
    if (!g_prof_on || g_prof_n >= kProfSlots) return;
    slot = g_prof_n++;
    if (slot >= g_prof_created) {
        (void)hipEventCreate(&g_prof_ev[slot][0]);
        (void)hipEventCreate(&g_prof_ev[slot][1]);
        g_prof_created = slot + 1;
    }
    g_prof_points[slot] = points;
    g_prof_kind[slot] = (kind >= 0 && kind < IDN_PROF_KINDS) ? kind : 0;
    (void)hipEventRecord(g_prof_ev[slot][0], s);
}
ProfScope::~ProfScope() {
    if (slot >= 0) (void)hipEventRecord(g_prof_ev[slot][1], s);
}

template <class T> static T* off(T* p, int64_t elems) { return p ? p + elems : p; }
// Where one compositing of the internal pass starting at ray r0 writes.  kCoarseFinal: the only compositing of a render without
// importance samples, into the render's maps; kCoarse: the one in front of a fine pass, into the *0 maps; kFine: the last one.
enum PassLevel { kCoarseFinal, kCoarse, kFine };
static idn_composite_out pass_out(const idn_render_args* a, int64_t r0, PassLevel level) {
    const bool c0 = level == kCoarse;
    idn_composite_out o = {};
    o.rgb_map = off(c0 ? a->rgb0 : a->rgb_map, r0 * 3);
    o.disp_map = off(c0 ? a->disp0 : a->disp_map, r0);
    o.acc_map = off(c0 ? a->acc0 : a->acc_map, r0);
    o.depth_map = c0 ? nullptr : off(a->depth_map, r0);
    o.weights = level == kFine ? off(a->tap_weights_fine, r0 * (a->n_samples + a->n_importance)) : off(a->tap_weights_coarse, r0 * a->n_samples);
    o.rgb_fg = off(c0 ? a->rgb_fg0 : a->rgb_fg, r0 * 3);
    o.last_weight = off(c0 ? a->last_weight0 : a->last_weight, r0);
    return o;
}

}  // namespace idn

using namespace idn;

extern "C" {

int idealnerf_version(void) { return 4; }   // 4: idn_render_args grew by `rng_mode / rng_seed / rng_ray0` (round 4); 3: by `fused_march`
const char* idealnerf_last_error(void) { return g_err; }

size_t idealnerf_packed_weight_floats(int precision) {
    // 4 bytes per weight (fp32, or bf16 hi + bf16 lo); 2 for the plain-bf16 stream
    if (precision == IDN_PREC_F32 || precision == IDN_PREC_BF16X3 || precision == IDN_PREC_FP16X3) return (size_t)kStreamFrags * kFragFloats;
    if (precision == IDN_PREC_BF16) return (size_t)kPlainStreamFrags * kFragFloats;
    if (precision == IDN_PREC_BF16X6) return (size_t)kX6StreamFrags * kFragFloats;   // three bf16 pieces per weight, 48-fragment slices
    return 0;
}
size_t idealnerf_folded_bias_floats(void) { return kBiasFloats; }

int idealnerf_pack_weights(const idn_facenerf_params* p, int precision, float* packed, void* stream) {
    if (int e = check_params(p)) return e;
    if (int e = check_precision(precision)) return e;
    if (!packed) return fail(IDN_EINVAL, "packed is NULL");
    if (precision == IDN_PREC_BF16X3) return launch_pack_bf16x3(*p, packed, (hipStream_t)stream);
    if (precision == IDN_PREC_FP16X3) return launch_pack_bf16x3(*p, packed, (hipStream_t)stream, 1);
    if (precision == IDN_PREC_BF16) return launch_pack_bf16(*p, packed, (hipStream_t)stream);
    if (precision == IDN_PREC_BF16X6) return launch_pack_bf16x6(*p, packed, (hipStream_t)stream);
    return launch_pack_f32(*p, packed, (hipStream_t)stream);
}

int idealnerf_fold_conditioning(const idn_facenerf_params* p, const float* aud, const float* expr,
                                const float* latent, float* folded, void* stream) {
    if (int e = check_params(p)) return e;
    if (!folded) return fail(IDN_EINVAL, "folded is NULL");
    if ((p->dim_aud > 0) != (aud != nullptr)) return fail(IDN_EINVAL, "aud pointer does not match dim_aud=%d", p->dim_aud);
    if ((p->dim_expr > 0) != (expr != nullptr)) return fail(IDN_EINVAL, "expr pointer does not match dim_expr=%d", p->dim_expr);
    if ((p->dim_latent > 0) != (latent != nullptr))
        return fail(IDN_EINVAL, "latent pointer does not match dim_latent=%d", p->dim_latent);
    return launch_fold(*p, aud, expr, latent, folded, (hipStream_t)stream);
}

int idealnerf_params_pts_ch(const idn_facenerf_params* p) {
    return p && p->multires_plus1 >= 0 && p->multires_plus1 <= IDN_MAX_MULTIRES + 1 ? pts_ch_of(*p) : -1;
}
int idealnerf_params_views_ch(const idn_facenerf_params* p) {
    return p && p->multires_views_plus1 >= 0 && p->multires_views_plus1 <= IDN_MAX_MULTIRES_VIEWS + 1 ? views_ch_of(*p) : -1;
}

int idealnerf_facenerf_fwd_ch(const float* packed, const float* folded, int precision, const float* x, int pts_ch, int views_ch,
                              int64_t n, float* out, void* stream) {
    if (int e = check_precision(precision)) return e;
    if (int e = check_widths(pts_ch, views_ch)) return e;
    if (n < 0) return fail(IDN_EINVAL, "n < 0");
    if (n == 0) return IDN_OK;
    if (!packed || !folded || !x || !out) return fail(IDN_EINVAL, "NULL pointer");
    return launch_mlp(precision, mlp_rows(packed, folded, x, pts_ch, views_ch, n, out), (hipStream_t)stream, MlpGate{});
}
int idealnerf_facenerf_fwd(const float* packed, const float* folded, int precision, const float* x, int64_t n,
                           float* out, void* stream) {
    return idealnerf_facenerf_fwd_ch(packed, folded, precision, x, IDN_PTS_CH, IDN_VIEWS_CH, n, out, stream);
}

int idealnerf_query_rays_fwd(const float* packed, const float* folded, int precision, const float* rays,
                             const float* z, int64_t n_rays, int n_samples, float* raw, void* stream) {
    if (int e = check_precision(precision)) return e;
    if (n_rays < 0 || n_samples < 1) return fail(IDN_EINVAL, "bad sizes n_rays=%lld n_samples=%d", (long long)n_rays, n_samples);
    if (n_rays == 0) return IDN_OK;
    if (!packed || !folded || !rays || !z || !raw) return fail(IDN_EINVAL, "NULL pointer");
    return launch_mlp(precision, mlp_rays(packed, folded, rays, z, n_rays, n_samples, raw), (hipStream_t)stream, MlpGate{});
}

int idealnerf_query_points_fwd(const float* packed, const float* folded, int precision, const float* pts,
                               const float* viewdirs, int64_t n_rays, int n_samples, float* raw, void* stream) {
    if (int e = check_precision(precision)) return e;
    if (n_rays < 0 || n_samples < 1) return fail(IDN_EINVAL, "bad sizes n_rays=%lld n_samples=%d", (long long)n_rays, n_samples);
    if (n_rays == 0) return IDN_OK;
    if (!packed || !folded || !pts || !viewdirs || !raw) return fail(IDN_EINVAL, "NULL pointer");
    return launch_mlp(precision, mlp_points(packed, folded, pts, viewdirs, n_rays, n_samples, raw), (hipStream_t)stream, MlpGate{});
}

int idealnerf_frame_rays(const float* c2w, int H, int W, float focal, float cx, float cy, float near_, float far_,
                         int row0, int nrows, float* rays_out, void* stream) {
    if (!c2w || !rays_out) return fail(IDN_EINVAL, "NULL pointer");
    if (H <= 0 || W <= 0 || row0 < 0 || nrows < 0 || row0 + nrows > H) return fail(IDN_EINVAL, "bad frame/rows");
    if (nrows == 0) return IDN_OK;
    return launch_frame_rays_pixels(c2w, H, W, focal, cx, cy, near_, far_, (int64_t)row0 * W, nrows * W, rays_out, (hipStream_t)stream);
}

int idealnerf_philox_uniform(uint64_t seed, int which, int64_t row0, int64_t n_rows, int n_cols, float* out, void* stream) {
    if (which != 0 && which != 1) return fail(IDN_EINVAL, "which %d (0 = stratified offsets, 1 = importance draws)", which);
    if (row0 < 0 || n_rows < 0 || n_cols < 0) return fail(IDN_EINVAL, "bad sizes");
    if (n_rows == 0 || n_cols == 0) return IDN_OK;
    if (!out) return fail(IDN_EINVAL, "NULL pointer");
    return launch_philox_uniform((unsigned long long)seed, which, row0, n_rows, n_cols, out, (hipStream_t)stream);
}

size_t idealnerf_sample_pixels_workspace_bytes(void) { return 4 * sizeof(int); }

int idealnerf_sample_pixels(const uint8_t* region_map, int H, int W, int n_rect, int n_outside, int n_mouth, int n_torso,
                            uint64_t seed, uint64_t draw, void* workspace, size_t workspace_bytes, int64_t* sel, void* stream) {
    const int counts[4] = {n_rect, n_outside, n_mouth, n_torso};
    static const char* const names[4] = {"rect", "outside", "mouth", "torso"};
    if (H <= 0 || W <= 0 || (int64_t)H * W > (1LL << 30)) return fail(IDN_EINVAL, "bad frame %d x %d", H, W);
    int64_t total = 0;
    for (int g = 0; g < 4; ++g) {
        if (counts[g] < 0) return fail(IDN_EINVAL, "negative %s count %d", names[g], counts[g]);
        if (counts[g] > IDN_SAMPLE_MAX_REGION)
            return fail(IDN_EUNSUPPORTED, "%s count %d exceeds IDN_SAMPLE_MAX_REGION = %d picks per region", names[g], counts[g],
                        IDN_SAMPLE_MAX_REGION);
        total += counts[g];
    }
    if (!region_map || !workspace || (total > 0 && !sel)) return fail(IDN_EINVAL, "NULL pointer");
    if (workspace_bytes < idealnerf_sample_pixels_workspace_bytes() || ((uintptr_t)workspace & 3u))
        return fail(IDN_EWORKSPACE, "workspace of %zu bytes (need %zu, int32-aligned)", workspace_bytes, idealnerf_sample_pixels_workspace_bytes());
    return launch_sample_pixels(region_map, H, W, counts, (unsigned long long)seed, (unsigned long long)draw, (int*)workspace,
                                (long long*)sel, (hipStream_t)stream);
}

int idealnerf_gather_rays(const int64_t* sel, int64_t n, const float* c2w, int H, int W, float focal, float cx, float cy,
                          const uint8_t* image, const uint8_t* background, const float* target_table, const float* background_table,
                          float* batch_rays, float* target_s, float* bc_rgb, void* stream) {
    if (H <= 0 || W <= 0 || (int64_t)H * W > (1LL << 30)) return fail(IDN_EINVAL, "bad frame %d x %d", H, W);
    if (n < 0 || n > 0x7fffffffLL / 8) return fail(IDN_EINVAL, "bad n %lld", (long long)n);
    if (n == 0) return IDN_OK;
    if (!sel || !c2w || !image || !background || !target_table || !background_table || !batch_rays || !target_s || !bc_rgb)
        return fail(IDN_EINVAL, "NULL pointer");
    return launch_gather_rays((const long long*)sel, n, c2w, nullptr, H, W, focal, cx, cy, image, background, target_table,
                              background_table, batch_rays, nullptr, target_s, bc_rgb, (hipStream_t)stream);
}

int idealnerf_gather_ray_pairs(const int64_t* sel, int64_t n, const float* c2w, const float* c2w_torso, int H, int W, float focal,
                               float cx, float cy, const uint8_t* image, const uint8_t* background, const float* target_table,
                               const float* background_table, float* batch_rays, float* batch_rays_torso, float* target_s,
                               float* bc_rgb, void* stream) {
    if (H <= 0 || W <= 0 || (int64_t)H * W > (1LL << 30)) return fail(IDN_EINVAL, "bad frame %d x %d", H, W);
    if (n < 0 || n > 0x7fffffffLL / 8) return fail(IDN_EINVAL, "bad n %lld", (long long)n);
    if (n == 0) return IDN_OK;
    if (!sel || !c2w || !c2w_torso || !image || !background || !target_table || !background_table || !batch_rays ||
        !batch_rays_torso || !target_s || !bc_rgb)
        return fail(IDN_EINVAL, "NULL pointer");
    return launch_gather_rays((const long long*)sel, n, c2w, c2w_torso, H, W, focal, cx, cy, image, background, target_table,
                              background_table, batch_rays, batch_rays_torso, target_s, bc_rgb, (hipStream_t)stream);
}

size_t idealnerf_frame_scores_workspace_bytes(int H, int W) { return frame_scores_workspace_bytes(H, W); }

int idealnerf_frame_scores(const float* pred, const uint8_t* truth, const uint8_t* regions, int H, int W, double* out,
                           void* workspace, size_t workspace_bytes, void* stream) {
    if (H <= 0 || W <= 0 || (int64_t)H * W > (1LL << 30)) return fail(IDN_EINVAL, "bad frame %d x %d", H, W);
    if (!pred || !truth || !out) return fail(IDN_EINVAL, "NULL pointer (pred, truth or out)");
    const size_t need = frame_scores_workspace_bytes(H, W);
    if (!workspace || workspace_bytes < need || ((uintptr_t)workspace & 7u))
        return fail(IDN_EINVAL, "workspace of %zu bytes (need %zu, 8-byte aligned)", workspace_bytes, need);
    return launch_frame_scores(pred, truth, regions, H, W, out, (double*)workspace, (hipStream_t)stream);
}

static int check_patches(int n_patches, int p) {
    if (n_patches < 1 || n_patches > IDN_PATCH_MAX) return fail(IDN_EINVAL, "n_patches %d is outside 1..%d", n_patches, IDN_PATCH_MAX);
    if (p < IDN_PATCH_MIN_P || p > IDN_PATCH_MAX_P)
        return fail(IDN_EINVAL, "patch edge %d is outside %d..%d", p, IDN_PATCH_MIN_P, IDN_PATCH_MAX_P);
    return IDN_OK;
}

int idealnerf_patch_pixels(const idn_patch_set* set, int W, int64_t* sel_out, void* stream) {
    if (!set || !sel_out) return fail(IDN_EINVAL, "NULL pointer");
    if (int e = check_patches(set->n_patches, set->p)) return e;
    if (W <= 0 || W > (1 << 15)) return fail(IDN_EINVAL, "bad frame width %d", W);
    for (int k = 0; k < set->n_patches; ++k)
        if (set->oy[k] < 0 || set->oy[k] > (1 << 15) || set->ox[k] < 0 || set->ox[k] + set->p > W)
            return fail(IDN_EINVAL, "patch %d at (%d, %d) with edge %d leaves a frame %d wide", k, set->oy[k], set->ox[k], set->p, W);
    return launch_patch_pixels(*set, W, (long long*)sel_out, (hipStream_t)stream);
}

int idealnerf_ssim_patch_fwd(const float* pred, const float* truth, int n_patches, int p, double* out, void* stream) {
    if (int e = check_patches(n_patches, p)) return e;
    if (!pred || !truth || !out) return fail(IDN_EINVAL, "NULL pointer (pred, truth or out)");
    if ((uintptr_t)out & 7u) return fail(IDN_EINVAL, "out is not 8-byte aligned");
    return launch_ssim_patch_fwd(pred, truth, n_patches, p, out, (hipStream_t)stream);
}

int idealnerf_ssim_patch_bwd(const float* pred, const float* truth, int n_patches, int p, float g, float* d_pred, void* stream) {
    if (int e = check_patches(n_patches, p)) return e;
    if (!pred || !truth || !d_pred) return fail(IDN_EINVAL, "NULL pointer (pred, truth or d_pred)");
    return launch_ssim_patch_bwd(pred, truth, n_patches, p, g, d_pred, (hipStream_t)stream);
}

int idealnerf_coarse_depths(const float* rays, const float* t_vals, const float* t_rand, int lindisp, int64_t n_rays,
                            int n_samples, float* z, void* stream) {
    if (n_rays < 0 || n_samples < 1) return fail(IDN_EINVAL, "bad sizes");
    if (n_rays == 0) return IDN_OK;
    if (!rays || !t_vals || !z) return fail(IDN_EINVAL, "NULL pointer");
    return launch_coarse_depths(rays, t_vals, t_rand, n_rays, n_samples, lindisp, z, Draws{}, (hipStream_t)stream);
}

size_t idealnerf_audio_net_saved_floats(int n_windows) { return audio_net_saved_floats(n_windows); }
int idealnerf_audio_net_fwd(const idn_audio_net_params* p, const float* windows, int n_windows, float* out, float* saved,
                            void* stream) {
    return launch_audio_net_fwd(p, windows, n_windows, out, saved, (hipStream_t)stream);
}
int idealnerf_audio_net_bwd(const idn_audio_net_params* p, const idn_audio_net_grads* grads, const float* windows,
                            const float* saved, const float* d_out, int n_windows, void* stream) {
    return launch_audio_net_bwd(p, grads, windows, saved, d_out, n_windows, (hipStream_t)stream);
}

int idealnerf_to8b(const float* rgb, int64_t n_pixels, int swap_rb, uint8_t* out, int* nonfinite_flag, void* stream) {
    if (n_pixels < 0) return fail(IDN_EINVAL, "n_pixels < 0");
    if (n_pixels == 0) return IDN_OK;
    if (!rgb || !out) return fail(IDN_EINVAL, "NULL pointer");
    return launch_to8b(rgb, n_pixels, swap_rb, out, nonfinite_flag, (hipStream_t)stream);
}

int idealnerf_compose_to8b(const float* rgb_head, const float* last_weight, const float* rgb_fg, int64_t n_pixels,
                           int swap_rb, uint8_t* out, uint8_t* fg_out, int* nonfinite_flag, void* stream) {
    if (n_pixels < 0) return fail(IDN_EINVAL, "n_pixels < 0");
    if (n_pixels == 0) return IDN_OK;
    if (!rgb_head || !last_weight || !rgb_fg || !out) return fail(IDN_EINVAL, "NULL pointer");
    return launch_compose_to8b(rgb_head, last_weight, rgb_fg, n_pixels, swap_rb, out, fg_out, nonfinite_flag,
                               (hipStream_t)stream);
}

int idealnerf_composite_fwd(const float* raw, const float* z, const float* rays, const float* bc_rgb,
                            const float* sigma_noise, int white_bkgd, int64_t n_rays, int n_samples,
                            const idn_composite_out* out, void* stream) {
    if (n_rays < 0) return fail(IDN_EINVAL, "n_rays < 0");
    if (n_rays == 0) return IDN_OK;
    if (!raw || !z || !rays || !bc_rgb || !out) return fail(IDN_EINVAL, "NULL pointer");
    return launch_composite(CompositeIn{raw, z, rays, bc_rgb, sigma_noise, white_bkgd, n_rays, n_samples}, *out, (hipStream_t)stream);
}

int idealnerf_sample_pdf_fwd(const float* z, const float* weights, const float* u, int u_per_ray, int64_t n_rays,
                             int n_samples, int n_importance, float* z_samples, int64_t* inds, float* cdf,
                             float* z_fine, float* z_std, void* stream) {
    if (n_rays < 0) return fail(IDN_EINVAL, "n_rays < 0");
    if (n_rays == 0) return IDN_OK;
    if (!z || !weights || !u) return fail(IDN_EINVAL, "NULL pointer");
    if (n_samples < 3) return fail(IDN_EUNSUPPORTED, "sample_pdf needs n_samples >= 3");
    SampleArgs s = sample_depths(z, weights, u, u_per_ray, n_rays, n_samples, n_importance);
    s.z_samples = z_samples; s.inds = inds; s.cdf_out = cdf; s.z_fine = z_fine; s.z_std = z_std;
    return launch_sample_pdf(s, (hipStream_t)stream);
}

int idealnerf_march_fwd(const float* raw, const float* z, const float* rays, const float* bc_rgb, const float* sigma_noise,
                        int white_bkgd, const float* u, int u_per_ray, int64_t n_rays, int n_samples, int n_importance,
                        const idn_composite_out* out, float* z_samples, int64_t* inds, float* cdf, float* z_fine,
                        float* z_std, void* stream) {
    if (n_rays < 0) return fail(IDN_EINVAL, "n_rays < 0");
    if (n_rays == 0) return IDN_OK;
    if (!raw || !z || !rays || !bc_rgb || !u || !out) return fail(IDN_EINVAL, "NULL pointer");
    const CompositeIn in = {raw, z, rays, bc_rgb, sigma_noise, white_bkgd, n_rays, n_samples};
    SampleArgs s = sample_march(in, u, u_per_ray, n_importance, Draws{});
    s.z_samples = z_samples; s.inds = inds; s.cdf_out = cdf; s.z_fine = z_fine; s.z_std = z_std;
    return launch_march(in, *out, s, (hipStream_t)stream);
}

int idealnerf_sample_pdf_bins_fwd(const float* bins, const float* weights, const float* u, int u_per_ray,
                                  int64_t n_rays, int n_bins, int n_importance, float* z_samples, int64_t* inds,
                                  float* cdf, void* stream) {
    if (n_rays < 0) return fail(IDN_EINVAL, "n_rays < 0");
    if (n_rays == 0) return IDN_OK;
    if (!bins || !weights || !u) return fail(IDN_EINVAL, "NULL pointer");
    SampleArgs s = sample_bins(bins, weights, u, u_per_ray, n_rays, n_bins, n_importance);
    s.z_samples = z_samples; s.inds = inds; s.cdf_out = cdf;
    return launch_sample_pdf(s, (hipStream_t)stream);
}

int idealnerf_invert_cdf(const float* cdf, const float* bins, const float* u, int u_per_ray, int64_t n_rays,
                         int n_bins, int n_importance, float* z_samples, int64_t* inds, void* stream) {
    if (n_rays < 0) return fail(IDN_EINVAL, "n_rays < 0");
    if (n_rays == 0) return IDN_OK;
    if (!cdf || !bins || !u) return fail(IDN_EINVAL, "NULL pointer");
    SampleArgs s = sample_cdf(cdf, bins, u, u_per_ray, n_rays, n_bins, n_importance);
    s.z_samples = z_samples; s.inds = inds;
    return launch_sample_pdf(s, (hipStream_t)stream);
}

size_t idealnerf_train_acts_floats(int64_t n_points) {
    if (n_points <= 0) return 0;
    return (size_t)((n_points + 127) / 128 * 128) * kActColsAll;
}

int idealnerf_query_rays_train_fwd(const float* packed, const float* folded, int precision, const float* rays,
                                   const float* z, int64_t n_rays, int n_samples, float* raw, float* acts,
                                   void* stream) {
    return idealnerf_query_rays_train_fwd_ch(packed, folded, precision, rays, z, n_rays, n_samples, IDN_PTS_CH, IDN_VIEWS_CH, raw, acts,
                                             stream);
}

int idealnerf_query_rays_train_fwd_ch(const float* packed, const float* folded, int precision, const float* rays,
                                      const float* z, int64_t n_rays, int n_samples, int pts_ch, int views_ch, float* raw,
                                      float* acts, void* stream) {
    if (int e = check_precision_train(precision)) return e;
    if (int e = check_widths(pts_ch, views_ch)) return e;
    if (n_rays < 0 || n_samples < 1) return fail(IDN_EINVAL, "bad sizes");
    if (n_rays == 0) return IDN_OK;
    if (!packed || !folded || !rays || !z || !raw || !acts) return fail(IDN_EINVAL, "NULL pointer");
    const int64_t p_pad = (n_rays * n_samples + 127) / 128 * 128;
    // (both activation-saving kernels write every row of the slab, the p_pad - n padding rows included -- they repeat the last
    //  point, and their deltas are zero: tests/test_hip_parity.py::test_train_forward_defines_every_row_of_the_activation_slab)
    return launch_mlp(precision, mlp_saving(mlp_rays(packed, folded, rays, z, n_rays, n_samples, raw), acts, p_pad, pts_ch, views_ch),
                      (hipStream_t)stream, MlpGate{});
}

size_t idealnerf_pass_bwd_workspace_bytes(int64_t n_rays, int n_samples) {
    if (n_rays <= 0 || n_samples <= 0) return 0;
    return bwd_workspace_bytes(n_rays * n_samples);
}

static int check_grads(const idn_facenerf_grads* grads) {
    if (!grads) return fail(IDN_EINVAL, "grads is NULL");
    for (int i = 0; i < 8; ++i)
        if (!grads->pts_w[i] || !grads->pts_b[i]) return fail(IDN_EINVAL, "grad pts_linears.%d is NULL", i);
    for (int i = 0; i < 3; ++i)
        if (!grads->views_w[i] || !grads->views_b[i]) return fail(IDN_EINVAL, "grad views_linears.%d is NULL", i);
    if (!grads->alpha_w || !grads->alpha_b || !grads->rgb_w || !grads->rgb_b) return fail(IDN_EINVAL, "grad head is NULL");
    return IDN_OK;
}

// The one host function behind the four pass-backward entries.  b.grads null: the frozen (conditioning-only) plan.
// Every argument error is answered here or at launch_pass_bwd's workspace check, before any HIP call.
static int pass_bwd_any(const PassBwd& b, void* stream) {
    const idn_facenerf_params* p = b.p;
    const BwdCond& c = b.cond;
    const bool frozen = !b.grads;
    if (int e = check_params(p)) return e;
    if (!frozen)
        if (int e = check_grads(b.grads)) return e;
    if ((p->dim_aud > 0) != (c.aud != nullptr) || (p->dim_expr > 0) != (c.expr != nullptr) ||
        (p->dim_latent > 0) != (c.latent != nullptr))
        return fail(IDN_EINVAL, "conditioning pointers do not match the widths");
    if (c.d_expr && (p->dim_expr == 0 || !c.expr)) return fail(IDN_EINVAL, "d_expr for a network without an expression");
    if (frozen && b.d_rays) return fail(IDN_EUNSUPPORTED, "the conditioning-only backward (grads NULL) returns no ray gradient");
    if (!frozen && c.d_vb) return fail(IDN_EINVAL, "d_views0_bias is the frozen plan's: with grads it is grads->views_b[0]");
    const bool want_cond = c.d_aud || c.d_latent || c.d_expr;
    if (frozen && c.d_vb && !want_cond) return fail(IDN_EINVAL, "d_views0_bias needs d_aud, d_latent or d_expr (with none the pass is not run)");
    if (b.n_rays < 0) return fail(IDN_EINVAL, "n_rays < 0");
    if (b.n_rays == 0 || (frozen && !want_cond)) return IDN_OK;   // nothing to deliver
    if (!b.acts || !b.raw || !b.z || !b.rays || !b.bc) return fail(IDN_EINVAL, "NULL pointer");
    return launch_pass_bwd(b, (hipStream_t)stream);
}
// idealnerf_pass_bwd and _rays have no frozen plan: a NULL grads is their error, behind the params' as in pass_bwd_any
static int pass_bwd_trained(const PassBwd& b, void* stream) {
    if (int e = check_params(b.p)) return e;
    if (!b.grads) return check_grads(b.grads);
    return pass_bwd_any(b, stream);
}

int idealnerf_pass_bwd(const idn_facenerf_params* p, const idn_facenerf_grads* grads, const float* aud,
                       const float* expr, const float* latent, const float* acts, const float* raw, const float* z,
                       const float* rays, const float* bc_rgb, int64_t n_rays, int n_samples, const float* g_rgb_map,
                       const float* g_rgb_fg, const float* g_last_weight, const float* g_acc, float* d_aud,
                       float* d_latent, void* workspace, size_t workspace_bytes, void* stream) {
    PassBwd b = {};
    b.p = p; b.grads = grads;
    b.cond.aud = aud; b.cond.expr = expr; b.cond.latent = latent; b.cond.d_aud = d_aud; b.cond.d_latent = d_latent;
    b.acts = acts; b.raw = raw; b.z = z; b.rays = rays; b.bc = bc_rgb; b.n_rays = n_rays; b.S = n_samples;
    b.g_rgb = g_rgb_map; b.g_fg = g_rgb_fg; b.g_lw = g_last_weight; b.g_acc = g_acc; b.ws = workspace; b.ws_bytes = workspace_bytes;
    return pass_bwd_trained(b, stream);
}

int idealnerf_pass_bwd_rays(const idn_facenerf_params* p, const idn_facenerf_grads* grads, const float* aud,
                            const float* expr, const float* latent, const float* acts, const float* raw, const float* z,
                            const float* rays, const float* bc_rgb, int64_t n_rays, int n_samples, const float* g_rgb_map,
                            const float* g_rgb_fg, const float* g_last_weight, const float* g_acc, float* d_aud,
                            float* d_latent, float* d_rays, void* workspace, size_t workspace_bytes, void* stream) {
    PassBwd b = {};
    b.p = p; b.grads = grads;
    b.cond.aud = aud; b.cond.expr = expr; b.cond.latent = latent; b.cond.d_aud = d_aud; b.cond.d_latent = d_latent;
    b.acts = acts; b.raw = raw; b.z = z; b.rays = rays; b.bc = bc_rgb; b.n_rays = n_rays; b.S = n_samples;
    b.g_rgb = g_rgb_map; b.g_fg = g_rgb_fg; b.g_lw = g_last_weight; b.g_acc = g_acc; b.ws = workspace; b.ws_bytes = workspace_bytes;
    b.d_rays = d_rays;
    return pass_bwd_trained(b, stream);
}

int idealnerf_pass_bwd_cond(const idn_facenerf_params* p, const float* aud, const float* expr, const float* latent,
                            const float* acts, const float* raw, const float* z, const float* rays, const float* bc_rgb,
                            int64_t n_rays, int n_samples, const float* g_rgb_map, const float* g_rgb_fg,
                            const float* g_last_weight, const float* g_acc, float* d_aud, float* d_latent, void* workspace,
                            size_t workspace_bytes, void* stream) {
    PassBwd b = {};
    b.p = p;
    b.cond.aud = aud; b.cond.expr = expr; b.cond.latent = latent; b.cond.d_aud = d_aud; b.cond.d_latent = d_latent;
    b.acts = acts; b.raw = raw; b.z = z; b.rays = rays; b.bc = bc_rgb; b.n_rays = n_rays; b.S = n_samples;
    b.g_rgb = g_rgb_map; b.g_fg = g_rgb_fg; b.g_lw = g_last_weight; b.g_acc = g_acc; b.ws = workspace; b.ws_bytes = workspace_bytes;
    return pass_bwd_any(b, stream);
}

int idealnerf_pass_bwd_ex(const idn_facenerf_params* p, const idn_facenerf_grads* grads, const float* aud,
                          const float* expr, const float* latent, const float* acts, const float* raw, const float* z,
                          const float* rays, const float* bc_rgb, int64_t n_rays, int n_samples, const float* g_rgb_map,
                          const float* g_rgb_fg, const float* g_last_weight, const float* g_acc, float* d_aud,
                          float* d_latent, const idn_pass_bwd_extra* extra, void* workspace, size_t workspace_bytes,
                          void* stream) {
    PassBwd b = {};
    b.p = p; b.grads = grads;
    b.cond.aud = aud; b.cond.expr = expr; b.cond.latent = latent; b.cond.d_aud = d_aud; b.cond.d_latent = d_latent;
    if (extra) b.cond.d_expr = extra->d_expr, b.cond.d_vb = extra->d_views0_bias, b.d_rays = extra->d_rays;
    b.acts = acts; b.raw = raw; b.z = z; b.rays = rays; b.bc = bc_rgb; b.n_rays = n_rays; b.S = n_samples;
    b.g_rgb = g_rgb_map; b.g_fg = g_rgb_fg; b.g_lw = g_last_weight; b.g_acc = g_acc; b.ws = workspace; b.ws_bytes = workspace_bytes;
    return pass_bwd_any(b, stream);
}

int idealnerf_facenerf_train_fwd(const float* packed, const float* folded, int precision, const float* x, int64_t n,
                                 float* out, float* acts, void* stream) {
    return idealnerf_facenerf_train_fwd_ch(packed, folded, precision, x, IDN_PTS_CH, IDN_VIEWS_CH, n, out, acts, stream);
}
int idealnerf_facenerf_train_fwd_ch(const float* packed, const float* folded, int precision, const float* x, int pts_ch,
                                    int views_ch, int64_t n, float* out, float* acts, void* stream) {
    if (int e = check_precision_train(precision)) return e;
    if (int e = check_widths(pts_ch, views_ch)) return e;
    if (n < 0) return fail(IDN_EINVAL, "n < 0");
    if (n == 0) return IDN_OK;
    if (!packed || !folded || !x || !out || !acts) return fail(IDN_EINVAL, "NULL pointer");
    if (n > 0x7fffffffLL) return fail(IDN_EUNSUPPORTED, "n %lld exceeds 2^31-1 per launch", (long long)n);
    const int64_t p_pad = (n + 127) / 128 * 128;
    return launch_mlp(precision, mlp_saving(mlp_rows(packed, folded, x, pts_ch, views_ch, n, out), acts, p_pad), (hipStream_t)stream,
                      MlpGate{});
}

size_t idealnerf_facenerf_bwd_workspace_bytes(int64_t n) {
    if (n <= 0) return 0;
    return bwd_workspace_bytes(n);
}

int idealnerf_facenerf_bwd(const idn_facenerf_params* p, const idn_facenerf_grads* grads, const float* aud, const float* expr,
                           const float* latent, const float* acts, int64_t n, const float* g_out, float* d_x, float* d_aud,
                           float* d_expr, float* d_latent, void* workspace, size_t workspace_bytes, void* stream) {
    if (int e = check_params(p)) return e;
    if (int e = check_grads(grads)) return e;
    if ((p->dim_aud > 0) != (aud != nullptr) || (p->dim_expr > 0) != (expr != nullptr) ||
        (p->dim_latent > 0) != (latent != nullptr))
        return fail(IDN_EINVAL, "conditioning pointers do not match the widths");
    if (n < 0) return fail(IDN_EINVAL, "n < 0");
    if (n == 0) return IDN_OK;
    if (!acts || !g_out) return fail(IDN_EINVAL, "NULL pointer");
    const BwdCond cond = {aud, expr, latent, d_aud, d_expr, d_latent, nullptr};   // (d_vb is the frozen pass plan's)
    return launch_facenerf_bwd(*p, *grads, cond, acts, n, g_out, d_x, workspace, workspace_bytes, (hipStream_t)stream);
}

size_t idealnerf_dw_gemm_workspace_bytes(void) { return dw_gemm_workspace_bytes(); }

int idealnerf_dw_gemm(const float* delta, int ld_delta, const float* acts, int ld_acts, int64_t rows, float* dW, float* db,
                      int pipe, void* workspace, size_t workspace_bytes, void* stream) {
    if (!delta || !acts || !dW) return fail(IDN_EINVAL, "NULL pointer");
    return launch_dw_gemm(delta, ld_delta, acts, ld_acts, rows, dW, db, pipe, workspace, workspace_bytes, (hipStream_t)stream);
}

size_t idealnerf_dw_products_workspace_bytes(void) { return dw_products_workspace_bytes(); }

int idealnerf_dw_products(int64_t rows, int pipe, int x6_items, idn_dw_product* products, int n, void* workspace,
                          size_t workspace_bytes, void* stream) {
    return launch_dw_products(rows, pipe, x6_items, products, n, workspace, workspace_bytes, (hipStream_t)stream);
}

size_t idealnerf_delta_chain_workspace_bytes(void) { return delta_chain_workspace_bytes(); }

int idealnerf_delta_chain(const idn_facenerf_params* p, int pipe, const float* acts, int64_t p_pad, const float* d_rgb,
                          float* dv0, float* dv21, float* da, int max_blocks, int* blocks_out, void* workspace,
                          size_t workspace_bytes, void* stream) {
    if (int e = check_params(p)) return e;
    return launch_delta_chain_alone(*p, pipe, acts, p_pad, d_rgb, dv0, dv21, da, max_blocks, blocks_out, workspace,
                                    workspace_bytes, (hipStream_t)stream);
}

int idealnerf_composite_bwd(const float* raw, const float* z, const float* rays, const float* bc_rgb, int64_t n_rays,
                            int n_samples, const float* g_rgb_map, const float* g_rgb_fg, const float* g_last_weight,
                            const float* g_acc, float* d_rgb, int ld_rgb, float* d_sig, int ld_sig, float* d_norm, int ld_norm,
                            void* stream) {
    if (n_rays < 0) return fail(IDN_EINVAL, "composite_bwd: n_rays < 0");
    if (n_rays == 0) return IDN_OK;
    if (!raw || !z || !rays || !bc_rgb || !d_rgb || !d_sig) return fail(IDN_EINVAL, "composite_bwd: NULL pointer");
    if ((uintptr_t)raw & 15) return fail(IDN_EINVAL, "composite_bwd: raw is not 16-byte aligned");
    if (ld_rgb < 3 || ld_sig < 1 || (d_norm && ld_norm < 1))
        return fail(IDN_EINVAL, "composite_bwd: row pitch %d / %d / %d below 3 / 1 / 1", ld_rgb, ld_sig, ld_norm);
    if (n_rays > 0x7fffffffLL) return fail(IDN_EUNSUPPORTED, "composite_bwd: n_rays %lld exceeds 2^31-1 per launch", (long long)n_rays);
    const CompBwdArgs a{reinterpret_cast<const float4*>(raw), z, rays, bc_rgb, g_rgb_map, g_rgb_fg, g_last_weight, g_acc,
                        d_rgb, ld_rgb, d_sig, ld_sig, (long)n_rays, n_samples, d_norm, ld_norm};
    return launch_composite_bwd(a, (hipStream_t)stream);
}

int idealnerf_input_grad(const idn_facenerf_params* p, const float* dA0, const float* dA5, const float* dV0, int64_t n,
                         int64_t p_pad, float* d_x, int max_blocks, int* blocks_out, void* stream) {
    if (int e = check_params(p)) return e;
    if (!dA0 || !dA5 || !dV0 || !d_x) return fail(IDN_EINVAL, "input_grad: NULL pointer");
    if (p_pad <= 0 || p_pad % 128) return fail(IDN_EINVAL, "input_grad: p_pad %lld is not a positive multiple of 128", (long long)p_pad);
    if (p_pad > (1LL << 24)) return fail(IDN_EUNSUPPORTED, "input_grad: p_pad %lld exceeds 2^24", (long long)p_pad);
    if (n < 1 || n > p_pad) return fail(IDN_EINVAL, "input_grad: n %lld outside [1, p_pad = %lld]", (long long)n, (long long)p_pad);
    if (max_blocks < 0) return fail(IDN_EINVAL, "input_grad: max_blocks %d < 0", max_blocks);
    if (((uintptr_t)dA0 | (uintptr_t)dA5 | (uintptr_t)dV0) & 15) return fail(IDN_EINVAL, "input_grad: the delta matrices are not 16-byte aligned");
    return launch_dx(*p, dA0, dA5, dV0, n, p_pad, d_x, max_blocks, blocks_out, (hipStream_t)stream);
}

int idealnerf_ray_grad(const float* d_x, int pts_ch, int views_ch, const float* rays, const float* z, int64_t n_rays, int n_samples,
                       float* d_rays, void* stream) {
    if (n_rays < 0) return fail(IDN_EINVAL, "ray_grad: n_rays < 0");
    if (n_rays == 0) return IDN_OK;
    if (!d_x || !rays || !z || !d_rays) return fail(IDN_EINVAL, "ray_grad: NULL pointer");
    if (!widths_ok(pts_ch, views_ch)) return fail(IDN_EINVAL, "ray_grad: row widths %d / %d", pts_ch, views_ch);
    if (n_samples < 2 || n_samples > 512) return fail(IDN_EUNSUPPORTED, "ray_grad: n_samples %d outside [2, 512]", n_samples);
    return launch_ray_grad(d_x, pts_ch, views_ch, rays, z, n_rays, n_samples, d_rays, (hipStream_t)stream);
}

int idealnerf_fold_bwd(const idn_facenerf_params* p, const float* aud, const float* expr, const float* latent, const float* db0,
                       const float* db5, const float* dbv, float* gW0, float* gW5, float* gWv0, float* d_aud, float* d_expr,
                       float* d_latent, void* stream) {
    if (int e = check_params(p)) return e;
    if ((p->dim_aud > 0) != (aud != nullptr) || (p->dim_expr > 0) != (expr != nullptr) || (p->dim_latent > 0) != (latent != nullptr))
        return fail(IDN_EINVAL, "fold_bwd: conditioning pointers do not match the widths");
    const int given = (gW0 != nullptr) + (gW5 != nullptr) + (gWv0 != nullptr);
    if (given != 0 && given != 3) return fail(IDN_EINVAL, "fold_bwd: %d of the three gradient tensors (all three, or none for the d cond range alone)", given);
    if ((d_aud && !p->dim_aud) || (d_expr && !p->dim_expr) || (d_latent && !p->dim_latent))
        return fail(IDN_EINVAL, "fold_bwd: a gradient for a conditioning vector the network does not have");
    if (p->dim_aud + p->dim_expr + p->dim_latent == 0) return IDN_OK;   // nothing to fold
    if (!db0 || !db5) return fail(IDN_EINVAL, "fold_bwd: NULL bias gradient");
    if (!dbv && p->dim_expr > 0 && (given || d_expr)) return fail(IDN_EINVAL, "fold_bwd: NULL bias gradient of views_linears.0");
    const FoldBwdArgs f{*p, aud, expr, latent, db0, db5, dbv, gW0, gW5, gWv0, d_aud, d_latent, d_expr};
    return launch_fold_bwd(f, given == 0, (hipStream_t)stream);
}

size_t idealnerf_cond_colsums_workspace_bytes(void) { return cond_colsums_workspace_bytes(); }

int idealnerf_cond_colsums(const float* dA0, const float* dA5, const float* dV0, int64_t P, int64_t p_pad, float* db, float* dbv,
                           void* workspace, size_t workspace_bytes, void* stream) {
    const int pts = (dA0 != nullptr) + (dA5 != nullptr) + (db != nullptr), views = (dV0 != nullptr) + (dbv != nullptr);
    if ((pts != 0 && pts != 3) || (views != 0 && views != 2))
        return fail(IDN_EINVAL, "cond_colsums: NULL pointer inside a pair (dA0, dA5, db come together, and dV0 with dbv)");
    if (p_pad <= 0 || p_pad % 128) return fail(IDN_EINVAL, "cond_colsums: p_pad %lld is not a positive multiple of 128", (long long)p_pad);
    if (p_pad > (1LL << 24)) return fail(IDN_EUNSUPPORTED, "cond_colsums: p_pad %lld exceeds 2^24", (long long)p_pad);
    if (P < 1 || P > p_pad) return fail(IDN_EINVAL, "cond_colsums: P %lld outside [1, p_pad = %lld]", (long long)P, (long long)p_pad);
    if (!pts && !views) return IDN_OK;
    if (!workspace || workspace_bytes < cond_colsums_workspace_bytes() || ((uintptr_t)workspace & 7))
        return fail(IDN_EWORKSPACE, "cond_colsums: workspace %zu < %zu (or not 8-byte aligned)", workspace_bytes, cond_colsums_workspace_bytes());
    return launch_cond_colsums(dA0, dA5, dV0, P, p_pad, db, dbv, reinterpret_cast<double*>(workspace), (hipStream_t)stream);
}

void idealnerf_profile_begin(void) {
    g_prof_n = 0;
    g_prof_on = true;
}

int idealnerf_profile_end_kinds(double* total_ms, int64_t* launches, int64_t* points) {
    g_prof_on = false;
    double ms[IDN_PROF_KINDS] = {0};
    int64_t n[IDN_PROF_KINDS] = {0}, pts[IDN_PROF_KINDS] = {0};
    for (int i = 0; i < g_prof_n; ++i) {
        IDN_HIP_CHECK(hipEventSynchronize(g_prof_ev[i][1]));
        float t = 0;
        IDN_HIP_CHECK(hipEventElapsedTime(&t, g_prof_ev[i][0], g_prof_ev[i][1]));
        const int k = g_prof_kind[i];
        ms[k] += t;
        n[k] += 1;
        pts[k] += g_prof_points[i];
    }
    for (int k = 0; k < IDN_PROF_KINDS; ++k) {
        if (total_ms) total_ms[k] = ms[k];
        if (launches) launches[k] = n[k];
        if (points) points[k] = pts[k];
    }
    return IDN_OK;
}

int idealnerf_profile_end(double* total_ms, int64_t* launches, int64_t* points) {
    double ms[IDN_PROF_KINDS];
    int64_t n[IDN_PROF_KINDS], pts[IDN_PROF_KINDS];
    if (int e = idealnerf_profile_end_kinds(ms, n, pts)) return e;
    // the forward MLP launches, with or without saved activations
    if (total_ms) *total_ms = ms[IDN_PROF_MLP_FWD] + ms[IDN_PROF_MLP_FWD_SAVE] + ms[IDN_PROF_MLP_FWD_SAVE_X6];
    if (launches) *launches = n[IDN_PROF_MLP_FWD] + n[IDN_PROF_MLP_FWD_SAVE] + n[IDN_PROF_MLP_FWD_SAVE_X6];
    if (points) *points = pts[IDN_PROF_MLP_FWD] + pts[IDN_PROF_MLP_FWD_SAVE] + pts[IDN_PROF_MLP_FWD_SAVE_X6];
    return IDN_OK;
}

// ---- render_rays --------------------------------------------------------------------
static const int64_t kRenderChunk = 32768;  // rays per internal pass (bounds the workspace)

static size_t align256(size_t x) { return (x + 255) & ~(size_t)255; }

struct RenderWs {
    float *z_c, *raw_c, *z_f, *raw_f;   // the compositing weights stay on chip (march kernel) or go straight to their tap
    size_t bytes;
};
static RenderWs carve(char* base, int64_t n, int S, int Ni) {
    RenderWs w;
    const int64_t c = n < kRenderChunk ? n : kRenderChunk;
    const int Sf = S + Ni;
    size_t off = 0;
    auto take = [&](size_t floats) {
        float* p = reinterpret_cast<float*>(base + off);
        off += align256(floats * sizeof(float));
        return p;
    };
    w.z_c = take((size_t)c * S);
    w.raw_c = take((size_t)c * S * 4);
    w.z_f = take((size_t)c * Sf);
    w.raw_f = take((size_t)c * Sf * 4);
    w.bytes = off;
    return w;
}

size_t idealnerf_render_workspace_bytes(int64_t n_rays, int n_samples, int n_importance) {
    if (n_rays <= 0 || n_samples <= 0 || n_importance < 0) return 0;
    return carve(nullptr, n_rays, n_samples, n_importance).bytes;
}

static int render_impl(const idn_render_args* a, const idn_frame* frame, const idn_render_opts* opts, void* stream_);
int idealnerf_render_rays_fwd(const idn_render_args* a, void* stream_) { return render_impl(a, nullptr, nullptr, stream_); }
int idealnerf_render_rays_fwd_opts(const idn_render_args* a, const idn_render_opts* opts, void* stream_) { return render_impl(a, nullptr, opts, stream_); }
float idealnerf_colour_gate_max_dist(void) { return kGateMaxDist; }

static size_t frame_scratch_bytes(int64_t n_rays) {
    const int64_t c = n_rays < kRenderChunk ? n_rays : kRenderChunk;
    return align256((size_t)c * IDN_RAY_FLOATS * sizeof(float));
}
size_t idealnerf_render_frame_workspace_bytes(int64_t n_rays, int n_samples, int n_importance) {
    const size_t base = idealnerf_render_workspace_bytes(n_rays, n_samples, n_importance);
    return base ? base + frame_scratch_bytes(n_rays) : 0;
}
int idealnerf_render_frame_fwd(const idn_render_args* a, const idn_frame* f, void* stream_) { return idealnerf_render_frame_fwd_opts(a, f, nullptr, stream_); }
int idealnerf_render_frame_fwd_opts(const idn_render_args* a, const idn_frame* f, const idn_render_opts* opts, void* stream_) {
    if (!a || !f) return fail(IDN_EINVAL, "args / frame is NULL");
    if (a->rays) return fail(IDN_EINVAL, "frame mode derives the rays from the camera: args->rays must be NULL");
    if (f->H <= 0 || f->W <= 0 || f->row0 < 0 || f->nrows < 0 || f->row0 + f->nrows > f->H) return fail(IDN_EINVAL, "bad frame / rows");
    if (a->n_rays != (int64_t)f->nrows * f->W) return fail(IDN_EINVAL, "n_rays %lld != nrows * W = %lld", (long long)a->n_rays, (long long)f->nrows * f->W);
    return render_impl(a, f, opts, stream_);
}

static int render_impl(const idn_render_args* a, const idn_frame* frame, const idn_render_opts* opts, void* stream_) {
    if (!a) return fail(IDN_EINVAL, "args is NULL");
    if (opts && opts->colour_gate != 0 && opts->colour_gate != 1) return fail(IDN_EINVAL, "colour_gate %d (1 = on, the default; 0 = off)", opts->colour_gate);
    if (int e = check_precision(a->precision)) return e;
    const int prec_fine = a->precision_fine_plus1 ? a->precision_fine_plus1 - 1 : a->precision;
    if (int e = check_precision(prec_fine)) return e;
    const int64_t n = a->n_rays;
    const int S = a->n_samples, Ni = a->n_importance, Sf = S + Ni;
    if (n < 0 || S < 2 || Ni < 0) return fail(IDN_EINVAL, "bad sizes n=%lld S=%d Ni=%d", (long long)n, S, Ni);
    if (n == 0) return IDN_OK;
    if ((!a->rays && !frame) || !a->bc_rgb || !a->t_vals || !a->packed_coarse || !a->folded_coarse)
        return fail(IDN_EINVAL, "NULL input pointer");
    if (a->rng_mode != 0 && a->rng_mode != 1) return fail(IDN_EINVAL, "rng_mode %d (0 = t_rand / u as tensors, 1 = drawn in the kernels)", a->rng_mode);
    if (a->rng_mode && (a->t_rand || a->u)) return fail(IDN_EINVAL, "rng_mode 1 draws t_rand and u in the kernels: both pointers must be NULL");
    if (a->rng_mode && a->rng_ray0 < 0) return fail(IDN_EINVAL, "rng_ray0 < 0");
    if (Ni > 0 && (!a->packed_fine || !a->folded_fine || (!a->u && !a->rng_mode))) return fail(IDN_EINVAL, "fine pass inputs are NULL");
    if (Ni > 0 && S < 3) return fail(IDN_EUNSUPPORTED, "importance sampling needs n_samples >= 3");
    const size_t need_base = idealnerf_render_workspace_bytes(n, S, Ni);
    const size_t need = need_base + (frame ? frame_scratch_bytes(n) : 0);
    if (!a->workspace || a->workspace_bytes < need)
        return fail(IDN_EWORKSPACE, "workspace %zu bytes < required %zu", a->workspace_bytes, need);
    float* const ray_scratch = frame ? reinterpret_cast<float*>(reinterpret_cast<char*>(a->workspace) + need_base) : nullptr;
    if (a->fused_march != 0 && a->fused_march != 1 && a->fused_march != 2) return fail(IDN_EINVAL, "fused_march %d (0 = kernel sequence, 1 = one kernel, 2 = two kernels)", a->fused_march);
    if (a->fused_march) {
        if (a->precision != IDN_PREC_F32 || prec_fine != IDN_PREC_F32) return fail(IDN_EUNSUPPORTED, "fused march: built for the fp32 arithmetic");
        if (S != 64 || Ni != 128) return fail(IDN_EUNSUPPORTED, "fused march: built for n_samples = 64, n_importance = 128 (got %d, %d)", S, Ni);
        if (a->noise_coarse || a->noise_fine) return fail(IDN_EUNSUPPORTED, "fused march: no density noise");
    }
    // the colour gate (include/idealnerf.h: idn_render_opts), pass by pass: fp32 only, and neither where noise is added to sigma
    // after the kernel nor where the raw colours themselves are asked for
    const bool gate_on = !opts || opts->colour_gate;
    const int gate_c = gate_on && a->precision == IDN_PREC_F32 && !a->noise_coarse && !a->tap_raw_coarse;
    const int gate_f = gate_on && prec_fine == IDN_PREC_F32 && !a->noise_fine && !a->tap_raw_fine;
    int64_t* const gate_counters = opts ? opts->gate_counters : nullptr;
    hipStream_t st = (hipStream_t)stream_;
    const RenderWs w = carve(reinterpret_cast<char*>(a->workspace), n, S, Ni);

    auto tap = [&](void* dst, const void* src, size_t bytes) -> int {
        if (!dst) return IDN_OK;
        IDN_HIP_CHECK(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToDevice, st));
        return IDN_OK;
    };

    for (int64_t r0 = 0; r0 < n; r0 += kRenderChunk) {
        const int64_t c = (n - r0 < kRenderChunk) ? n - r0 : kRenderChunk;
        const float* rays = frame ? ray_scratch : a->rays + r0 * IDN_RAY_FLOATS;
        if (frame) {   // this pass's records: pixels [row0 W + r0, .. + c) of the frame, into the scratch the pass before has finished with
            if (int e = launch_frame_rays_pixels(frame->c2w, frame->H, frame->W, frame->focal, frame->cx, frame->cy, frame->near_, frame->far_,
                                                 (int64_t)frame->row0 * frame->W + r0, (int)c, ray_scratch, st))
                return e;
            if (frame->rays_out)
                IDN_HIP_CHECK(hipMemcpyAsync(frame->rays_out + r0 * IDN_RAY_FLOATS, ray_scratch, (size_t)c * IDN_RAY_FLOATS * sizeof(float),
                                             hipMemcpyDeviceToDevice, st));
        }
        const float* bc = a->bc_rgb + r0 * 3;
        const Draws draws{(unsigned long long)a->rng_seed, (long)(a->rng_ray0 + r0), a->rng_mode};   // this pass's rows of the draw table
        // this pass's rows of u and of every tap
        const float* const u = a->u_per_ray ? off(a->u, r0 * Ni) : a->u;
        float* const tap_z_c = off(a->tap_z_coarse, r0 * S);
        float* const tap_raw_c = off(a->tap_raw_coarse, r0 * S * 4);
        float* const tap_z_samples = off(a->tap_z_samples, r0 * Ni);
        int64_t* const tap_inds = off(a->tap_inds, r0 * Ni);
        float* const tap_cdf = off(a->tap_cdf, r0 * (S - 1));
        float* const z_std = off(a->z_std, r0);
        float* const tap_z_f = off(a->tap_z_fine, r0 * Sf);
        float* const tap_raw_f = off(a->tap_raw_fine, r0 * Sf * 4);
        if (int e = launch_coarse_depths(rays, a->t_vals, off(a->t_rand, r0 * S), c, S, a->lindisp, w.z_c, draws, st)) return e;
        if (!a->fused_march)
            if (int e = launch_mlp(a->precision, mlp_rays(a->packed_coarse, a->folded_coarse, rays, w.z_c, c, S, w.raw_c), st, MlpGate{gate_c, gate_counters}))
                return e;
        const bool fine = Ni > 0;
        const idn_composite_out co = pass_out(a, r0, fine ? kCoarse : kCoarseFinal);
        if (int e = tap(tap_z_c, w.z_c, (size_t)c * S * 4)) return e;
        if (a->fused_march) {   // one kernel from the coarse depths to the pixels; raw, weights, cdf and the fine depths stay in LDS
            const bool split = a->fused_march == 2;   // two launches: the fine depths cross HBM (w.z_f), everything else stays on chip
            FusedArgs f = {};
            f.wstream_c = a->packed_coarse; f.bias_c = a->folded_coarse; f.wstream_f = a->packed_fine; f.bias_f = a->folded_fine;
            f.rays = rays; f.bc = bc; f.z_c = w.z_c; f.u = u; f.u_per_ray = a->u_per_ray; f.n_rays = (long)c; f.white_bkgd = a->white_bkgd;
            f.co = co; f.fo = pass_out(a, r0, kFine); f.z_std = z_std; f.draws = draws;
            f.tap_raw_c = tap_raw_c; f.tap_raw_f = tap_raw_f; f.tap_inds = tap_inds; f.tap_z_samples = tap_z_samples; f.tap_cdf = tap_cdf;
            if (split) f.z_f = w.z_f;
            else f.tap_z_fine = tap_z_f;
            if (int e = launch_render_fused(a->fused_march, f, st)) return e;
            if (split)
                if (int e = tap(tap_z_f, w.z_f, (size_t)c * Sf * 4)) return e;
            continue;
        }
        if (int e = tap(tap_raw_c, w.raw_c, (size_t)c * S * 16)) return e;
        const CompositeIn in_c = {w.raw_c, w.z_c, rays, bc, off(a->noise_coarse, r0 * S), a->white_bkgd, c, S};
        if (!fine) {
            if (int e = launch_composite(in_c, co, st)) return e;
            continue;
        }
        // the march between the passes: coarse compositing, inverse-CDF sampling and the merge in one kernel
        SampleArgs sm = sample_march(in_c, u, a->u_per_ray, Ni, draws);
        sm.z_samples = tap_z_samples; sm.inds = tap_inds; sm.cdf_out = tap_cdf; sm.z_fine = w.z_f; sm.z_std = z_std;
        if (int e = launch_march(in_c, co, sm, st)) return e;
        if (int e = launch_mlp(prec_fine, mlp_rays(a->packed_fine, a->folded_fine, rays, w.z_f, c, Sf, w.raw_f), st,
                               MlpGate{gate_f, gate_counters ? gate_counters + 2 : nullptr}))
            return e;
        if (int e = launch_composite(CompositeIn{w.raw_f, w.z_f, rays, bc, off(a->noise_fine, r0 * Sf), a->white_bkgd, c, Sf}, pass_out(a, r0, kFine), st)) return e;
        if (int e = tap(tap_z_f, w.z_f, (size_t)c * Sf * 4)) return e;
        if (int e = tap(tap_raw_f, w.raw_f, (size_t)c * Sf * 16)) return e;
    }
    return IDN_OK;
}

// ---- ray cull (cull.hip) -----------------------------------------------------------------
static int check_cull_G(int G) {
    if (G < 32 || G > 1024 || G % 32) return fail(IDN_EINVAL, "G = %d: the grid edge is a multiple of 32 in 32..1024", G);
    return IDN_OK;
}
static int check_cull_frame(const idn_frame* f) {
    if (!f) return fail(IDN_EINVAL, "frame is NULL");
    if (f->H <= 0 || f->W <= 0 || f->row0 < 0 || f->nrows < 0 || f->row0 + f->nrows > f->H) return fail(IDN_EINVAL, "bad frame/rows");
    if ((int64_t)f->nrows * f->W > 0x7fffffffLL) return fail(IDN_EUNSUPPORTED, "more than 2^31-1 pixels in one band");
    return IDN_OK;
}

int idealnerf_cull_mark(const float* raw, int64_t n, float sigma_min, uint8_t* corners, void* stream) {
    if (n < 0) return fail(IDN_EINVAL, "n < 0");
    if (n == 0) return IDN_OK;
    if (!raw || !corners) return fail(IDN_EINVAL, "NULL pointer");
    return launch_cull_mark(raw, n, sigma_min, corners, (hipStream_t)stream);
}

int idealnerf_cull_cells(const uint8_t* corners, int G, int dilate, uint32_t* bits, void* stream) {
    if (int e = check_cull_G(G)) return e;
    if (dilate < 0) return fail(IDN_EINVAL, "dilate %d < 0", dilate);
    if (!corners || !bits) return fail(IDN_EINVAL, "NULL pointer");
    return launch_cull_cells(corners, G, dilate > G ? G : dilate, bits, (hipStream_t)stream);
}

size_t idealnerf_cull_classify_workspace_bytes(int64_t n_pixels) { return n_pixels > 0 ? cull_classify_workspace_bytes(n_pixels) : 0; }

int idealnerf_cull_classify(const idn_cull_grid* grid, const idn_frame* frame, float dz, int K, int64_t* sel, int32_t* n_live,
                            void* workspace, size_t workspace_bytes, void* stream) {
    if (!grid) return fail(IDN_EINVAL, "grid is NULL");
    if (int e = check_cull_G(grid->G)) return e;
    if (int e = check_cull_frame(frame)) return e;
    if (!(grid->cell > 0.0f)) return fail(IDN_EINVAL, "cell must be positive");
    if (!(dz > 0.0f) || K < 1 || K > (1 << 20)) return fail(IDN_EINVAL, "march of K = %d steps of dz = %g (K in 1..2^20, dz > 0)", K, (double)dz);
    if (!grid->bits || !n_live) return fail(IDN_EINVAL, "NULL pointer");
    const int64_t npix = (int64_t)frame->nrows * frame->W;
    if (npix == 0) {
        IDN_HIP_CHECK(hipMemsetAsync(n_live, 0, sizeof(int32_t), (hipStream_t)stream));
        return IDN_OK;
    }
    if (!sel || !workspace) return fail(IDN_EINVAL, "NULL pointer");
    if (workspace_bytes < cull_classify_workspace_bytes(npix))
        return fail(IDN_EWORKSPACE, "workspace of %zu bytes, the classification of %lld pixels needs %zu", workspace_bytes, (long long)npix,
                    cull_classify_workspace_bytes(npix));
    return launch_cull_classify(*grid, *frame, dz, K, (long long*)sel, n_live, workspace, (hipStream_t)stream);
}

int idealnerf_cull_gather(const int64_t* sel, int64_t n, const idn_frame* frame, const float* bc, float* rays, float* bc_live,
                          void* stream) {
    if (int e = check_cull_frame(frame)) return e;
    if (n < 0 || n > (int64_t)frame->nrows * frame->W) return fail(IDN_EINVAL, "n = %lld is not in 0..nrows W", (long long)n);
    if (n == 0) return IDN_OK;
    if (!sel || !bc || !rays || !bc_live) return fail(IDN_EINVAL, "NULL pointer");
    return launch_cull_gather((const long long*)sel, n, *frame, bc, rays, bc_live, (hipStream_t)stream);
}

int idealnerf_cull_scatter(const int64_t* sel, int64_t n_live, int64_t n_pixels, const float* bc, const idn_cull_output* outputs,
                           int n_outputs, void* stream) {
    if (n_pixels < 0 || n_live < 0 || n_live > n_pixels) return fail(IDN_EINVAL, "bad sizes n_live=%lld n_pixels=%lld", (long long)n_live, (long long)n_pixels);
    if (n_outputs < 0 || n_outputs > IDN_CULL_MAX_OUTPUTS) return fail(IDN_EINVAL, "n_outputs %d outside 0..%d", n_outputs, IDN_CULL_MAX_OUTPUTS);
    if (n_outputs > 0 && !outputs) return fail(IDN_EINVAL, "NULL pointer");
    for (int k = 0; k < n_outputs; ++k) {
        const idn_cull_output& o = outputs[k];
        if (o.channels != 1 && o.channels != 3) return fail(IDN_EINVAL, "output %d: channels %d (1 or 3)", k, o.channels);
        if (o.fill_background && (o.channels != 3 || !bc)) return fail(IDN_EINVAL, "output %d: the background fill needs 3 channels and bc", k);
        if (!o.dense || (n_live > 0 && !o.live)) return fail(IDN_EINVAL, "output %d: NULL pointer", k);
    }
    if (n_live > 0 && !sel) return fail(IDN_EINVAL, "NULL pointer");
    if (n_pixels == 0 || n_outputs == 0) return IDN_OK;
    return launch_cull_scatter((const long long*)sel, n_live, n_pixels, bc, outputs, n_outputs, (hipStream_t)stream);
}

// ---- sample cull of the live rays (cull.hip) ----------------------------------------------
static int check_cull_points(int64_t n, int S) {
    if (n < 0 || S < 1) return fail(IDN_EINVAL, "bad sizes n=%lld S=%d", (long long)n, S);
    if (n * (int64_t)S > 0x7fffffffLL) return fail(IDN_EUNSUPPORTED, "more than 2^31-1 points in one call (n = %lld, S = %d)", (long long)n, S);
    return IDN_OK;
}

int idealnerf_cull_sample_classify(const idn_cull_grid* grid, const float* rays, const float* z, int64_t n, int S, int64_t* sel,
                                   int32_t* n_live, void* workspace, size_t workspace_bytes, void* stream) {
    if (!grid) return fail(IDN_EINVAL, "grid is NULL");
    if (int e = check_cull_G(grid->G)) return e;
    if (int e = check_cull_points(n, S)) return e;
    if (!(grid->cell > 0.0f)) return fail(IDN_EINVAL, "cell must be positive");
    if (!grid->bits || !n_live) return fail(IDN_EINVAL, "NULL pointer");
    const int64_t n_points = n * S;
    if (n_points == 0) {
        IDN_HIP_CHECK(hipMemsetAsync(n_live, 0, sizeof(int32_t), (hipStream_t)stream));
        return IDN_OK;
    }
    if (!rays || !z || !sel || !workspace) return fail(IDN_EINVAL, "NULL pointer");
    if (workspace_bytes < cull_classify_workspace_bytes(n_points))
        return fail(IDN_EWORKSPACE, "workspace of %zu bytes, the classification of %lld points needs %zu", workspace_bytes,
                    (long long)n_points, cull_classify_workspace_bytes(n_points));
    return launch_cull_sample_classify(*grid, rays, z, n_points, S, (long long*)sel, n_live, workspace, (hipStream_t)stream);
}

int idealnerf_cull_sample_gather(const int64_t* sel, int64_t m, const float* rays, const float* z, int64_t n, int S, float* pts,
                                 float* dirs, void* stream) {
    if (int e = check_cull_points(n, S)) return e;
    if (m < 0 || m > n * S) return fail(IDN_EINVAL, "m = %lld is not in 0..n S", (long long)m);
    if (m == 0) return IDN_OK;
    if (!sel || !rays || !z || !pts || !dirs) return fail(IDN_EINVAL, "NULL pointer");
    return launch_cull_sample_gather((const long long*)sel, m, rays, z, n * S, S, pts, dirs, (hipStream_t)stream);
}

int idealnerf_cull_sample_scatter(const int64_t* sel, int64_t m, const float* raw_live, int64_t n_points, float* raw, void* stream) {
    if (n_points < 0 || m < 0 || m > n_points) return fail(IDN_EINVAL, "bad sizes m=%lld n_points=%lld", (long long)m, (long long)n_points);
    if (n_points > 0x7fffffffLL) return fail(IDN_EUNSUPPORTED, "more than 2^31-1 points in one call");
    if (n_points == 0) return IDN_OK;
    if (!raw || (m > 0 && (!sel || !raw_live))) return fail(IDN_EINVAL, "NULL pointer");
    if (((uintptr_t)raw | (uintptr_t)raw_live) & 15) return fail(IDN_EINVAL, "raw and raw_live must be 16-byte aligned (rows of four floats)");
    return launch_cull_sample_scatter((const long long*)sel, m, raw_live, n_points, raw, (hipStream_t)stream);
}

}  // extern "C"
