// Dispatch of the fused chain kernel (chain2_kernel.h): the one list of the configurations it is compiled for.  Each (Legendre
// order, ipc4d dtype) is one instantiation of rip_launch_chain2 in a translation unit of its own (chain_np*.hip), so that they
// compile in parallel.
#include "rip_common.h"

template <int NP, typename KT>
int rip_launch_chain2(rip_ctx *ctx, const RipPlan *plan, const ChainArgs &a);

typedef int (*ChainLauncher)(rip_ctx *ctx, const RipPlan *plan, const ChainArgs &a);

// 4 / 9 / 11 Legendre planes (P_ORDER 3 / 8 / 10), f32 or f64 ipc4d, 6, 8 or 16 groups (C2Form has a form for each); null for
// everything else (the stage kernels)
static ChainLauncher chain_launcher(int nplanes, int G, int k_dtype) {
    if (G != 6 && G != 8 && G != 16) return nullptr;
    const bool k64 = k_dtype == RIP_F64;
    switch (nplanes) {
        case 4:
            return k64 ? rip_launch_chain2<4, double> : rip_launch_chain2<4, float>;
        case 9:
            return k64 ? rip_launch_chain2<9, double> : rip_launch_chain2<9, float>;
        case 11:
            return k64 ? rip_launch_chain2<11, double> : rip_launch_chain2<11, float>;
    }
    return nullptr;
}

// f32 gain and a configuration listed above
bool rip_chain_supported(const rip_ctx *ctx, int nplanes, int G, int k_dtype, int gain_dtype) {
    (void)ctx;
    return gain_dtype == RIP_F32 && chain_launcher(nplanes, G, k_dtype);
}

// The f64-ipc4d form of up to 8 groups (C2Form, narrow = 1) fills the 160 KB of LDS of every CU with its partial K ring: the
// pre-pass of the next ramp finds no room beside it.  (Also true for the f64 group counts below 8 that have no fused form.)
bool rip_chain_fills_lds(int G, int k_dtype) { return k_dtype == RIP_F64 && G <= 8; }

// returns the launch status, or 1 when no fused kernel fits this plan / CALDIR set (the caller then takes the stage kernels)
int rip_launch_chain(rip_ctx *ctx, const RipPlan *plan, const ChainArgs &a, int nplanes, int k_dtype) {
    const ChainLauncher launch = chain_launcher(nplanes, a.ngrp, k_dtype);
    // (merged_dq < 0: this CALDIR set's flag words cannot be merged, RipCal)
    if (!launch || !ctx->use_chain2 || a.merged_dq < 0) return 1;
    const int rc = launch(ctx, plan, a);
    if (rc != 1) ctx->last_form = 2;
    return rc;
}
