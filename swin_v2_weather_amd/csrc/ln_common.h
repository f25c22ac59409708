// LayerNorm pieces shared by the fused row kernels (mlp.hip, proj_ln.hip).  Only what compiles to the SAME instruction streams as the
// written-out form lives here.  The forward epilogue, the backward's per-row rule and the fold of its d gamma / d beta sums were tried as
// functions too and are still written out in both kernels: LABNOTES.md, "Shared row-kernel rules: what could be written once".
#pragma once
#include "common.h"

namespace {

// LayerNorm backward in row layout: LPR lanes per row (4 columns each), the workgroup's ROWS rows in NPASS passes of RPP rows, the loads
// of BATCH passes in flight together.  (mlp_bwd_kernel, proj_ln_bwd_kernel)
template <int C, int NTHR, int ROWS>
struct LnBwdShape {
    static constexpr int LPR = C <= 32 ? 8 : C <= 64 ? 16 : C <= 128 ? 32 : 64;      // lanes per row (power of two >= C / 4)
    static constexpr int RPP = NTHR / LPR, NPASS = ROWS / RPP;
    static constexpr int BATCH = NPASS < 4 ? NPASS : 4;
    static_assert(NPASS % BATCH == 0, "row passes must come in whole batches");
};

}  // namespace
