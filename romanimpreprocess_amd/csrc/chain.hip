// Dispatch of the fused chain kernel (chain2_kernel.h): the one list of the configurations it is compiled for.  Each (Legendre
// order, ipc4d dtype, part of the group-count list) is one instantiation of rip_launch_chain2 in a translation unit of its own
// (chain_np*.hip, compiled once per part), so that they compile in parallel.
#include <string.h>

#include "chain2_form.h"

template <int NP, typename KT, int PART>
int rip_launch_chain2(rip_ctx *ctx, const RipPlan *plan, const ChainArgs &a, bool skip0);

typedef int (*ChainLauncher)(rip_ctx *ctx, const RipPlan *plan, const ChainArgs &a, bool skip0);

// part of the group-count list (rip_common.h: RIP_CHAIN_G_PART*) that holds G, -1 when the fused kernel has no form for G
static int chain_part(int G) {
#define RIP_IN_PART(g) \
    if (G == g) return part;
    int part = 0;
    RIP_CHAIN_G_PART0(RIP_IN_PART)
    part = 1;
    RIP_CHAIN_G_PART1(RIP_IN_PART)
    part = 2;
    RIP_CHAIN_G_PART2(RIP_IN_PART)
#undef RIP_IN_PART
    return -1;
}

template <int NP, typename KT>
static ChainLauncher chain_launcher_of(int part) {
    switch (part) {
        case 0:
            return rip_launch_chain2<NP, KT, 0>;
        case 1:
            return rip_launch_chain2<NP, KT, 1>;
        case 2:
            return rip_launch_chain2<NP, KT, 2>;
    }
    return nullptr;
}

// 4 / 9 / 11 Legendre planes (P_ORDER 3 / 8 / 10), f32 or f64 ipc4d, 5 to 16 groups (C2Form has a form for each even count; an odd
// count runs the form of the next even one); null for everything else (the stage kernels)
static ChainLauncher chain_launcher(int nplanes, int G, int k_dtype) {
    const int part = chain_part(G);
    if (part < 0 || (k_dtype != RIP_F32 && k_dtype != RIP_F64)) return nullptr;
    const bool k64 = k_dtype == RIP_F64;
    switch (nplanes) {
        case 4:
            return k64 ? chain_launcher_of<4, double>(part) : chain_launcher_of<4, float>(part);
        case 9:
            return k64 ? chain_launcher_of<9, double>(part) : chain_launcher_of<9, float>(part);
        case 11:
            return k64 ? chain_launcher_of<11, double>(part) : chain_launcher_of<11, float>(part);
    }
    return nullptr;
}

// f32 gain and a configuration listed above
bool rip_chain_supported(const rip_ctx *ctx, int nplanes, int G, int k_dtype, int gain_dtype) {
    (void)ctx;
    return gain_dtype == RIP_F32 && chain_launcher(nplanes, G, k_dtype);
}

// Context-free form of the same question for callers (include/romanhip.h): 2 = a fused form is compiled for this configuration,
// 0 = the stage kernels run
int rip_chain_form_for(int lin_nplanes, int ngroups, int ipc_dtype, int gain_dtype) {
    return rip_chain_supported(nullptr, lin_nplanes, ngroups, ipc_dtype, gain_dtype) ? 2 : 0;
}

// The launch geometry the fused kernel would use for such a ramp on a (ny, nx) frame, on a device of ncu CUs with the options
// "chain_reserve" = reserve and "chain_quad" = quad_ok: host arithmetic only, the launcher's own (c2_form_geometry).  0 = no
// fused form (or no such frame: the chain takes ny >= 16 and nx a multiple of the channel width), 2 = out filled.
int rip_chain_geometry_for(int lin_nplanes, int ngroups, int ipc_dtype, int gain_dtype, int ny, int nx, int ncu, int reserve,
                           int quad_ok, int out[8]) {
    if (!out || !rip_chain_form_for(lin_nplanes, ngroups, ipc_dtype, gain_dtype)) return 0;
    if (ny < 16 || nx < RIP_CW || nx % RIP_CW || ncu < 1) return 0;
    ChainArgs a;
    memset(&a, 0, sizeof a);
    a.ny = ny, a.nx = nx, a.ngrp = ngroups;
    if (reserve < 0) reserve = 0;   // as rip_set_option stores it
    const bool k64 = ipc_dtype == RIP_F64;
#define RIP_GEO(g)                                                                                   \
    if (ngroups == g) {                                                                              \
        if (k64)                                                                                     \
            c2_form_geometry<C2Form<g + (g & 1), true>>(a, ncu, reserve, quad_ok != 0, out);         \
        else                                                                                         \
            c2_form_geometry<C2Form<g + (g & 1), false>>(a, ncu, reserve, quad_ok != 0, out);        \
        return 2;                                                                                    \
    }
    RIP_CHAIN_G_ALL(RIP_GEO)
#undef RIP_GEO
    return 0;
}

// Does the fused form of this ramp fill the LDS of every CU, so that the pre-pass of the next ramp finds no room beside it?  From
// the form table: true for the form family whose K ring grows into what the rest of the layout leaves of the 160 KB (narrow = 1:
// f64 ipc4d with 5 to 8 groups).  That the pre-pass does better in front of its own ramp there was measured at f64 x 8 groups
// (profiles/r04_summary.md); 5, 6 and 7 groups inherit it with the form.  The family is the criterion, not a byte count: its
// forms leave under 7 KB, every other form at least 10 KB (asserted below, so that a layout change that moves a form across
// comes to notice).  Group counts WITHOUT a fused form keep the answer they always had (f64 ipc4d and up to 8 groups: true), so
// that the stage-kernel path of those ramps is scheduled exactly as before.
template <int GE, bool K64>
static constexpr bool c2_fills_lds() {
    using F = C2Form<GE, K64>;
    static_assert((F::narrow == 1) == (160 * 1024 - F::lds_bytes < 7 * 1024), "the K-ring forms, and only they, fill the LDS");
    return F::narrow == 1;
}
bool rip_chain_fills_lds(int G, int k_dtype) {
    if (chain_part(G) < 0 || (k_dtype != RIP_F32 && k_dtype != RIP_F64)) return k_dtype == RIP_F64 && G <= 8;
    const bool k64 = k_dtype == RIP_F64;
#define RIP_FILLS(g) \
    if (G == g) return k64 ? c2_fills_lds<g + (g & 1), true>() : c2_fills_lds<g + (g & 1), false>();
    RIP_CHAIN_G_ALL(RIP_FILLS)
#undef RIP_FILLS
    return false;
}

// returns the launch status, or 1 when no fused kernel fits this plan / CALDIR set (the caller then takes the stage kernels)
int rip_launch_chain(rip_ctx *ctx, const RipPlan *plan, const ChainArgs &a, int nplanes, int k_dtype, bool skip0) {
    const ChainLauncher launch = chain_launcher(nplanes, a.ngrp, k_dtype);
    // (merged_dq < 0: this CALDIR set's flag words cannot be merged, RipCal)
    if (!launch || !ctx->use_chain2 || a.merged_dq < 0) return 1;
    const int rc = launch(ctx, plan, a, skip0);
    if (rc != 1) ctx->last_form = 2, ctx->last_first_group = skip0 ? 1 : 0, ctx->last_bias_stream = a.bias_records ? 1 : 0;
    return rc;
}

// The conditions under which rip_launch_chain above and the launcher (chain2_kernel.h: launch_chain2, launch_chain2_s) run the
// fused kernel, restated so that a caller can know it BEFORE the pre-pass (which then leaves group 0's tables out), plus what
// the plan must be for group 0 to be dead in the fit: an excluded first group that is the single read 0 (no linearity flag
// from it), exactly the full set of tested differences from group 1 on, and the weight zero for group 0 in every variant.
bool rip_chain_may_skip_first(const rip_ctx *ctx, const RipPlan *plan, int nplanes, int G, int k_dtype, int gain_dtype, int merged_dq,
                              int nb) {
    if (!ctx->skip_first || !ctx->use_fused || !ctx->use_chain2 || !plan || merged_dq < 0 || nb < 2) return false;
    if (!rip_chain_supported(ctx, nplanes, G, k_dtype, gain_dtype)) return false;
    return plan->h.start == 1 && plan->h.do_not_flag_first && plan->k0_zero && plan->dense.valid == rip_full_valid_of(G, 1);
}
