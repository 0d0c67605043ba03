// Table of instantiations and plan executor of the INV variants of cc_fwd_bf16_kernel (cc_fwd_bf16_kernel.h), shared by the bracket
// search (cc_invert.hip, INV = 1: one tile = one sample) and the Newton solve (cc_solve.hip, INV = 2: one tile = sixteen rows).  The
// including file defines INV_MODE (that INV value), INV_WHAT ("invert" | "solve") and INV_ROWS (its name table in cc_fwd_plan.h)
// first; like it, this header is compiled twice, on bf16 pieces and (-DUMNN_FWD_PIECE_F16) on fp16 pieces.  Variants, names, image
// layouts, arithmetic mode and launch rules are cc_fwd_plan.h's (fwd_plan_inverse); the launch sequence is cc_fwd_launch.h's.
#pragma once
#include "cc_fwd_bf16_kernel.h"
#include "cc_fwd_launch.h"
using namespace UMNN_FWD_NS;

typedef void (*inv_kernel_t)(const FwdBf16Args);
#define INV_FN(T, NP, PP, EX, NR, PIPE, TREST, WPB, INV) cc_fwd_bf16_kernel<T, NP, PP, (EX) != 0, NR, (PIPE) != 0, INV, TREST, WPB>,
static const inv_kernel_t kInvKernels[] = {             // (in the order of INV_ROWS: a plan's variant is an index into both)
    UMNN_INV_ROWS_2(INV_FN, INV_MODE) UMNN_INV_ROWS_WIDE_FIRST(INV_FN, INV_MODE)
#ifndef UMNN_FWD_PIECE_F16
    UMNN_INV_ROWS_3(INV_FN, INV_MODE)
#endif
};
static_assert(sizeof(kInvKernels) / sizeof(kInvKernels[0]) == fwd_count(INV_ROWS), "one kernel per variant");
#ifdef UMNN_FWD_PIECE_F16
constexpr int INV_BUILD_F16 = 1;
#else
constexpr int INV_BUILD_F16 = 0;
#endif

// Executes a plan on this build; the caller has filled the operand fields of a zeroed FwdBf16Args (NI, d, E, n included).  ovf: bf16
// build only -- non-null = the queued fallback of an fp16-piece launch.  queue_bf16(second) queues the bf16 build of the same job, with
// the same plan, behind the launch of the fp16 build.
template <class QueueBf16>
static int inv_launch(const FwdPlan& pl, FwdBf16Args& args, double flops, hipStream_t stream, const UmnnOvfPlan* ovf, QueueBf16 queue_bf16) {
    const bool mine = ovf ? !INV_BUILD_F16 && pl.nparts == 2 : pl.f16 == INV_BUILD_F16;
    if (!mine || pl.error || pl.variant < 0 || pl.variant >= fwd_count(INV_ROWS)) return umnn_fail(UMNN_EUNSUPPORTED, kFwdPlanError);
    return umnn_fwd_launch_pieces(kInvKernels[pl.variant], pl, args, flops, "cc_" INV_WHAT " launch", stream, ovf, queue_bf16);
}
