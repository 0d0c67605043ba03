// Backward of the quadrature on the bf16 matrix cores: variant table and launcher of the one-pass kernels and the workgroup
// pipelines (the kernel templates, with their layout notes, live in cc_bwd_*_kernel.h; cc_bwd_bf16_kernel.h is shared with the
// three-stage backward of cc_backward_front.hip).  Which of them a call runs is decided in cc_bwd_plan.h; this file executes.
#include "cc_bwd_plan.h"

// ------------------------------------------------------------------------------------------
#define BWD_LOOP_ROW(LHH, NR, ...) { BWD_KIND_LOOP, LHH, NR, cc_bwd_bf16_kernel<LHH, true, NR> },
#define BWD_SWP_ROW(LHH, NR, ...) { BWD_KIND_SWP, LHH, NR, cc_bwd_swp_kernel<LHH, NR> },
#define BWD_WS_ROW(LHH, NR, ...) { BWD_KIND_WS, LHH, NR, cc_bwd_ws_kernel<NR> },
#define BWD_WS16_ROW(LHH, NR, ...) { BWD_KIND_WS16, LHH, NR, cc_bwd_ws16_kernel<NR> },
#define BWD_MID_WS16_ROW(LHH, NR, ...) { BWD_KIND_MID_WS16, LHH, NR, cc_bwd_ws16_kernel<NR, true> },
static const BwdBf16Variant kBwdBf16Variants[] = {
    UMNN_BWD_LOOP_SHAPES(BWD_LOOP_ROW, )
    UMNN_BWD_LOOP_SHAPES(BWD_SWP_ROW, )        // software-pipelined loop (cc_bwd_swp_kernel.h): same variants, same results, one shared W / W^T image
    UMNN_BWD_WS_SHAPES(BWD_WS_ROW, )           // weight-stationary workgroup pipeline (cc_bwd_ws_kernel.h)
    UMNN_BWD_WS_SHAPES(BWD_WS16_ROW, )         // the same on fp16 pieces (cc_bwd_ws16_kernel.h): three-term recompute, scaled cotangents, overflow flag + queued fallback
    UMNN_BWD_WS_SHAPES(BWD_MID_WS16_ROW, )     // ... as the middle stage of the three-stage backward (cc_backward_front.hip launches it through umnn_ws16_mid_launch)
};
static_assert(offsetof(Ws16Scal, flag) == 3 * sizeof(unsigned), "cc_backward_front.hip addresses the flag as scal + 3");

int umnn_ws16_prepare(const BwdArgs& base, unsigned cotmax_blocks, hipStream_t stream) {
    if (int rc = umnn_check(hipMemsetAsync(base.scal, 0, sizeof(Ws16Scal), stream), "memset launch scalars")) return rc;
    hipLaunchKernelGGL(cc_bwd_cotmax_kernel<>, dim3(cotmax_blocks), dim3(256), 0, stream, base, reinterpret_cast<Ws16Scal*>(base.scal));
    return 0;
}
int umnn_ws16_mid_launch(const BwdBf16Args& mid, int nrl, int nblocks, size_t lds_bytes, hipStream_t stream) {
    const bwd_bf16_kernel_t fn = bwd_bf16_fn(kBwdBf16Variants, BWD_KIND_MID_WS16, 4, nrl);
    if (!fn) return umnn_fail(UMNN_EINVAL, kBwdRouteError);
    if (int rc = umnn_allow_lds((const void*)fn, lds_bytes)) return rc;
    hipLaunchKernelGGL(fn, dim3(nblocks), dim3(64 * WS_WAVES), lds_bytes, stream, mid);
    return 0;
}

// -DUMNN_WS_TIMING builds: per-role step times of one pipeline launch (the kernel writes six doubles per wave through args.tz2).
// ws_timing_arm ahead of the launch, ws_timing_report behind it (synchronises the stream).
static void ws_timing_arm(BwdBf16Args& args, int nblocks, hipStream_t stream) {
#ifdef UMNN_WS_TIMING
    static double* tbuf = nullptr;
    if (!tbuf) hipMalloc(&tbuf, sizeof(double) * 6 * 8192);
    hipMemsetAsync(tbuf, 0, sizeof(double) * 6 * nblocks * WS_WAVES, stream);
    args.tz2 = reinterpret_cast<const float*>(tbuf);
#endif
}
static void ws_timing_report(BwdBf16Args& args, const char* tag, int nblocks, hipStream_t stream) {
#ifdef UMNN_WS_TIMING
    const int nw = nblocks * WS_WAVES;
    hipStreamSynchronize(stream);
    static double host[6 * 8192];
    hipMemcpy(host, args.tz2, sizeof(double) * 6 * nw, hipMemcpyDeviceToHost);
    const char* role[8] = {"Ca", "F1", "F2", "F3", "Cb", "B1", "B2", "B3"};
    for (int r = 0; r < WS_WAVES; ++r) {
        double sm[6] = {0};
        for (int w = r; w < nw; w += WS_WAVES) for (int j = 0; j < 6; ++j) sm[j] += host[6 * w + j];
        const double st = sm[4] > 0 ? sm[4] : 1;
        fprintf(stderr, "%s %s per step (s_memtime ticks): prep %.0f | work to the %d %% mark %.0f | rest of the work %.0f | barrier wait %.0f   (steps per wave %.0f)\n",
                tag, role[r], sm[0] / st, UMNN_WS_TRACE_FRAC, sm[1] / st, sm[2] / st, sm[3] / st, sm[4] / (nw / WS_WAVES));
    }
    args.tz2 = nullptr;
#endif
}

// Launches the main backward pass of a BWD_FAMILY_WS16 / WS / SWP / LOOP route.
int umnn_launch_backward_bf16(const BwdArgs& base, const umnn_mlp* net, const BwdRoute& rt, hipStream_t stream) {
    BwdBf16Args args;
    args.b = base;
    args.z2 = nullptr; args.d2 = nullptr; args.tz2 = nullptr; args.grp0 = 0; args.nl2 = 0; args.accumulate = 0;
    args.scal = nullptr; args.only_if = nullptr;
    BwdArgs& a = args.b;
    a.ns = rt.ns;
    a.l_lo = 1;
    const int kind = rt.family == BWD_FAMILY_SWP ? BWD_KIND_SWP : rt.family == BWD_FAMILY_LOOP ? BWD_KIND_LOOP : BWD_KIND_WS;
    const bwd_bf16_kernel_t fn = bwd_bf16_fn(kBwdBf16Variants, kind, rt.L, rt.nrl);
    const bwd_bf16_kernel_t fn16 = rt.family == BWD_FAMILY_WS16 ? bwd_bf16_fn(kBwdBf16Variants, BWD_KIND_WS16, rt.L, rt.nrl) : nullptr;
    if (rt.family < BWD_FAMILY_WS16 || rt.family > BWD_FAMILY_LOOP || !fn || (rt.family == BWD_FAMILY_WS16 && !(fn16 && a.scal)))
        return umnn_fail(UMNN_EINVAL, kBwdRouteError);
    if (rt.family == BWD_FAMILY_LOOP) bwd_onepass_images(rt.L, NPB, &args);
    if (int rc = umnn_allow_lds((const void*)fn, rt.lds_bytes)) return rc;
    const dim3 grid(rt.nblocks), block(64 * rt.wpb);
    const double flops = umnn_bwd_flops(net, a.n, a.NI);
    switch (rt.family) {
    case BWD_FAMILY_WS16:
        // cotangent scale first, then the pipeline, then the bf16 pipeline queued behind it as the fallback that only runs if a
        // piece overflowed (same outputs, rewritten)
        if (int rc = umnn_allow_lds((const void*)fn16, rt.lds16_bytes)) return rc;
        args.scal = a.scal;
        {
            int rc_prepare = 0;
            const int rc = umnn_bwd_launch(stream, flops, rt.name, "cc_bwd_f16 (ws) launch", [&] {
                if ((rc_prepare = umnn_ws16_prepare(a, rt.cotmax_blocks, stream))) return;
                ws_timing_arm(args, rt.nblocks, stream);
                hipLaunchKernelGGL(fn16, grid, block, rt.lds16_bytes, stream, args);
                ws_timing_report(args, "WS16_TIMING", rt.nblocks, stream);
                args.only_if = &reinterpret_cast<Ws16Scal*>(a.scal)->flag;
                hipLaunchKernelGGL(fn, grid, block, rt.lds_bytes, stream, args);
            });
            return rc_prepare ? rc_prepare : rc;
        }
    case BWD_FAMILY_WS:
        return umnn_bwd_launch(stream, flops, rt.name, "cc_bwd_bf16 (ws) launch", [&] {
            ws_timing_arm(args, rt.nblocks, stream);
            hipLaunchKernelGGL(fn, grid, block, rt.lds_bytes, stream, args);
            ws_timing_report(args, "WS_TIMING", rt.nblocks, stream);
        });
    default:
        return umnn_bwd_launch(stream, flops, rt.name, rt.family == BWD_FAMILY_SWP ? "cc_bwd_bf16 (swp) launch" : "cc_bwd_bf16 launch",
                               [&] { hipLaunchKernelGGL(fn, grid, block, rt.lds_bytes, stream, args); });
    }
}
