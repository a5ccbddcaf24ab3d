// The fused kernel for 9 Legendre planes and f64 ipc4d coefficients (chain2_kernel.h; dispatch: chain.hip).
#include "chain2_kernel.h"

#ifndef C2_PART
#error "compiled once per part of the group-count list: -DC2_PART=0, 1, 2 (Makefile)"
#endif
template int rip_launch_chain2<9, double, C2_PART>(rip_ctx *ctx, const RipPlan *plan, const ChainArgs &a, bool skip0);
