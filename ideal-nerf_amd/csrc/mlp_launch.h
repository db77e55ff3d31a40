// The host side of a network-forward launch, once for every arithmetic.  A kernel file describes its family as an MlpKernels
// table -- which (mode, saving) instantiations it builds, with their dynamic LDS, and the tile and block geometry -- and its
// launcher is the table, the family's LaunchSetup and one call of launch_mlp_kernels.
#pragma once
#include "mlp_common.h"
#include "tile_order.h"

namespace idn {

struct MlpKernels {
    struct Cell {
        void (*kernel)(MlpArgs);   // null: the family does not build this combination
        int lds;                   // dynamic LDS bytes
    };
    Cell cell[3][2];               // [kModeRays / kModeX / kModePts][saving activations]
    void (*gated)(MlpGateArgs);    // the colour-gated rays-mode inference kernel, or null
    int gated_lds;
    int tile_points, threads;      // points per tile (grid = min(tiles, CUs)) and threads per block
    int prof_kind_saving;          // ProfScope kind of a saving launch; an inference launch is IDN_PROF_MLP_FWD
    const char* no_saving;         // the error text for a saving launch the family does not build
};

// a family of the three inference kernels alone, all with the same LDS
inline MlpKernels mlp_inference_kernels(void (*rays)(MlpArgs), void (*x)(MlpArgs), void (*pts)(MlpArgs), int lds, int tile_points, int threads) {
    MlpKernels k = {};
    k.cell[kModeRays][0] = {rays, lds}; k.cell[kModeX][0] = {x, lds}; k.cell[kModePts][0] = {pts, lds};
    k.tile_points = tile_points; k.threads = threads;
    k.prof_kind_saving = IDN_PROF_MLP_FWD;
    k.no_saving = "the activation-saving forward is built for IDN_PREC_F32 and IDN_PREC_BF16X6";
    return k;
}

inline int launch_mlp_kernels(const MlpKernels& k, LaunchSetup& setup, const MlpArgs& a, MlpGate gate, hipStream_t s) {
    if (a.n_points <= 0) return IDN_OK;
    const int mode = a.x ? kModeX : a.pts ? kModePts : kModeRays;
    const bool saving = a.acts != nullptr;
    if (gate.on && (saving || mode != kModeRays || !k.gated))
        return fail(IDN_EUNSUPPORTED, "the colour gate is built for the rays-mode inference launch");
    if ((mode == kModeX || saving) && !widths_ok(a.x_pts_ch, a.x_views_ch))
        return fail(IDN_EINVAL, "row widths %d / %d outside 3 + 6 L, L <= %d / %d", a.x_pts_ch, a.x_views_ch, IDN_MAX_MULTIRES, IDN_MAX_MULTIRES_VIEWS);
    const MlpKernels::Cell& c = k.cell[mode][saving];
    if (!c.kernel) return fail(IDN_EUNSUPPORTED, "%s", k.no_saving);
    int num_cu = 0;
    if (int e = setup.get([&k]() -> int {   // every instantiation of the family, on the first launch on a device
            for (const auto& row : k.cell)
                for (const MlpKernels::Cell& i : row)
                    if (i.kernel)
                        IDN_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(i.kernel), hipFuncAttributeMaxDynamicSharedMemorySize, i.lds));
            if (k.gated)
                IDN_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(k.gated), hipFuncAttributeMaxDynamicSharedMemorySize, k.gated_lds));
            return IDN_OK;
        }, &num_cu))
        return e;
    const int64_t ntiles = (a.n_points + k.tile_points - 1) / k.tile_points;
    const int grid = (int)(ntiles < num_cu ? ntiles : num_cu);
    ProfScope prof(s, a.n_points, saving ? k.prof_kind_saving : IDN_PROF_MLP_FWD);
    if (gate.on) {
        MlpGateArgs ga;
        static_cast<MlpArgs&>(ga) = a;
        ga.gate_counters = reinterpret_cast<unsigned long long*>(gate.counters);
        ga.tile_step = tile_order_step(grid);
        hipLaunchKernelGGL(k.gated, dim3(grid), dim3(k.threads), k.gated_lds, s, ga);
    } else {
        hipLaunchKernelGGL(c.kernel, dim3(grid), dim3(k.threads), c.lds, s, a);
    }
    IDN_HIP_CHECK(hipGetLastError());
    return IDN_OK;
}

}  // namespace idn
