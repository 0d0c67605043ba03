// Executing a forward-class plan (cc_fwd_plan.h), once for every family and job: the forward on fp32 MFMA, on pieces and on the
// 32x32x16 kernel, the bracket search, the Newton solve.
//
// Overflow protocol of the fp16-piece launches (the library default).  An fp16 piece overflows at 65520; the value it belongs to then
// reaches the quadrature sum of its integral as inf / NaN (every product with an inf piece is inf or NaN and nothing downstream can
// make it finite again).  The fp16 build therefore checks that sum once per tile group, in the epilogue: a group with a non-finite sum
// writes NOTHING but a NaN marker into its output slots, raises the launch's flag word, and leaves its integrals to the bf16 build of
// the same kernel (bf16 pieces share fp32's exponent range), which is queued right behind the fp16 launch WITH THE SAME PLAN -- build,
// overflow mode and function pointer are all that differ.  That second launch costs one scalar load per workgroup when the flag is
// down (every benchmarked net); when it is up it recomputes exactly the marked groups -- on two bf16 pieces, i.e. those integrals
// come back at bf16x3 accuracy (~6e-6) instead of ~5e-7 -- and publishes them, the one-pass log-likelihood rows included (a deferred
// group has not counted towards its rows yet).  NaN inputs take the same road and come back NaN.  Flag words: a per-device ring of
// 64-bit words, launch generation g uses word g % 256, raised with atomicMax(word, g), tested as word >= g -- no memset between
// launches, safe across streams, and a replayed hipGraph (g baked into its nodes) at worst runs a fallback that finds no marked group.
#pragma once
#include "cc_fwd_plan.h"
#include "cc_fwd_shared.h"

// the snapshot of the forward options a plan is made from
inline FwdOptions umnn_fwd_options() {
    const UmnnOptions& o = umnn_options();
    return FwdOptions{o.fwd_precision, o.fwd_p, o.fwd_ns, o.fwd_tail, o.fwd_pipe, o.fwd_pad, o.fwd_pad_min};
}

// One launch of a plan.  args: the kernel's argument block, f the FwdArgs inside it (operands filled by the caller; the plan's net,
// split and grid and the overflow fields are written here).  ovf: null, or -- bf16 build only -- this launch is the queued fallback
// of an fp16-piece launch: no profiling bracket, no launch note.  queue_bf16(second): queues that fallback (called by the fp16 launch
// of a plan with one, inside its bracket).
template <class Kernel, class Args, class QueueBf16>
inline int umnn_fwd_launch(Kernel fn, const FwdPlan& pl, Args& args, FwdArgs& f, double flops, const char* what, hipStream_t stream,
                           const UmnnOvfPlan* ovf, QueueBf16&& queue_bf16) {
    UmnnOvfPlan own{0, nullptr, 0};
    const bool queues = pl.fallback && !ovf;
    if (queues) {
        own.mode = 1;
        if (int rc = umnn_ovf_slot(&own.flag, &own.gen)) return rc;
    }
    if (!ovf) ovf = &own;
    f.m = pl.m; f.ns = pl.ns; f.ngroups = pl.ngroups;
    f.ovf_mode = ovf->mode; f.ovf_flag = ovf->flag; f.ovf_gen = ovf->gen;
    if (int rc = umnn_allow_lds((const void*)fn, pl.lds_bytes)) return rc;
    const bool queued = ovf->mode == 2;
    if (!queued) umnn_prof_begin(stream);
    hipLaunchKernelGGL(fn, dim3(pl.blocks), dim3(pl.block), pl.lds_bytes, stream, args);
    int rc = umnn_check(hipGetLastError(), what);
    if (!rc && queues) rc = queue_bf16(UmnnOvfPlan{2, own.flag, own.gen});
    if (!queued) {
        umnn_prof_end(stream, flops);
        umnn_note_launch(pl.name);
    }
    return rc;
}
inline int umnn_fwd_no_fallback(const UmnnOvfPlan&) { return 0; }

// ... of a piece kernel (FwdBf16Args of either build): the plan's image layout goes into the arguments first
template <class Kernel, class Args, class QueueBf16>
inline int umnn_fwd_launch_pieces(Kernel fn, const FwdPlan& pl, Args& args, double flops, const char* what, hipStream_t stream,
                                  const UmnnOvfPlan* ovf, QueueBf16&& queue_bf16) {
    for (int l = 0; l < UMNN_MAX_LINEAR; ++l) {
        args.pl.ks32[l] = pl.img.ks32[l]; args.pl.off16[l] = pl.img.off16[l]; args.pl.half_in[l] = pl.img.half_in[l];
    }
    return umnn_fwd_launch(fn, pl, args, args.f, flops, what, stream, ovf, queue_bf16);
}
