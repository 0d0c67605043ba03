// Forward quadrature on the 16-bit matrix cores: the table of instantiations and the launcher of a plan.  The kernel template, with its
// layout notes, lives in cc_fwd_bf16_kernel.h and is shared with the search and the solve (cc_inv_launch.h); variants, names, image
// layouts and every launch rule are cc_fwd_plan.h's; the launch sequence and the overflow protocol are cc_fwd_launch.h's.
#ifndef UMNN_ASM_TIED
#define UMNN_ASM_TIED 1      // cc_common.h: inline-assembly outputs tied to inputs in the forward translation units
#endif
#include "cc_fwd_bf16_kernel.h"
#include "cc_fwd_launch.h"
using namespace UMNN_FWD_NS;
// (this file is compiled twice: as is -- bf16 pieces, umnn_launch_forward_bf16 -- and through cc_forward_f16.hip with
// -DUMNN_FWD_PIECE_F16 -- fp16 pieces, umnn_launch_forward_f16, kernel names cc_fwd_f16<...>)
#ifdef UMNN_FWD_PIECE_F16
#define FWD_ROWS kFwdRowsF16
#define FWD_WHAT "cc_fwd_f16 launch"
#define FWD_LAUNCH umnn_launch_forward_f16
#define FWD_BUILD_F16 1
#else
#define FWD_ROWS kFwdRowsBf16
#define FWD_WHAT "cc_fwd_bf16 launch"
#define FWD_LAUNCH umnn_launch_forward_bf16
#define FWD_BUILD_F16 0
#endif

typedef void (*fwd_bf16_kernel_t)(const FwdBf16Args);
#define FWD_FN(T, NP, PP, EX, NR, PIPE, TREST, WPB, INV) cc_fwd_bf16_kernel<T, NP, PP, (EX) != 0, NR, (PIPE) != 0, INV, TREST, WPB>,
static const fwd_bf16_kernel_t kFwdKernels[] = {        // (in the order of FWD_ROWS: a plan's variant is an index into both)
    UMNN_FWD_ROWS_2(FWD_FN, 0) UMNN_FWD_ROWS_WIDE_FIRST(FWD_FN, 0)
#ifndef UMNN_FWD_PIECE_F16
    UMNN_FWD_ROWS_3(FWD_FN, 0)
#endif
};
static_assert(sizeof(kFwdKernels) / sizeof(kFwdKernels[0]) == fwd_count(FWD_ROWS), "one kernel per variant");

int umnn_launch_forward_bf16(const FwdPlan& pl, const FwdArgs& a, double flops, hipStream_t stream, const UmnnOvfPlan* ovf);

// Executes a plan of the piece families on this build.  ovf (bf16 build only): non-null = the queued fallback of an fp16-piece
// launch, which hands over its own plan.
int FWD_LAUNCH(const FwdPlan& pl, const FwdArgs& a, double flops, hipStream_t stream, const UmnnOvfPlan* ovf) {
    const bool mine = ovf ? !FWD_BUILD_F16 && pl.nparts == 2 : pl.f16 == FWD_BUILD_F16;
    if (!mine || (pl.family != FWD_FAMILY_PIECES && pl.family != FWD_FAMILY_WIDE_FIRST) || pl.variant < 0 || pl.variant >= fwd_count(FWD_ROWS))
        return umnn_fail(UMNN_EUNSUPPORTED, kFwdPlanError);
    FwdBf16Args args{};
    args.f = a;
    return umnn_fwd_launch_pieces(kFwdKernels[pl.variant], pl, args, flops, FWD_WHAT, stream, ovf,
                                  [&](const UmnnOvfPlan& second) { return umnn_launch_forward_bf16(pl, a, flops, stream, &second); });
}
