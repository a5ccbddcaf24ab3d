// The fused kernel for 4 Legendre planes and f64 ipc4d coefficients (chain2_kernel.h; dispatch: chain.hip).
#include "chain2_kernel.h"

template int rip_launch_chain2<4, double>(rip_ctx *ctx, const RipPlan *plan, const ChainArgs &a);
