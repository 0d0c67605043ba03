// Variant tables and launcher of the INV variants of cc_fwd_bf16_kernel (cc_fwd_bf16_kernel.h), shared by the bracket search
// (cc_invert.hip, INV = 1: one tile = one sample) and the Newton solve (cc_solve.hip, INV = 2: one tile = sixteen rows).  The
// including file defines INV_MODE (that INV value) and INV_KNAME (the prefix of its kernel names) first; like it, this header is
// compiled twice, on bf16 pieces and (-DUMNN_FWD_PIECE_F16) on fp16 pieces.  The weight images are the forward's (cc_fwd_plan.h);
// the plan is its P = 1 subset, except that 3..4-tile nets are always padded and uniform wide nets may run on any piece count.
#pragma once
#include "cc_fwd_plan.h"
using namespace UMNN_FWD_NS;

struct InvOvfPlan { int mode; unsigned long long* flag; unsigned long long gen; };
int umnn_ovf_slot(unsigned long long** flag, unsigned long long* gen);                                  // cc_api.hip

typedef void (*inv_kernel_t)(const FwdBf16Args);
struct InvVariant { int tmax, exact, nrl, nparts, wpb; inv_kernel_t fn; const char* name; };
#define INV_VARIANT(T, EX, NR) { T, EX, NR, 2, 4, cc_fwd_bf16_kernel<T, 2, 1, (EX) != 0, NR, false, INV_MODE>, INV_KNAME "<T=" #T ",EXACT=" #EX ",LIVE=" #NR ">" }
// (eight waves per workgroup: images that leave room for one workgroup per CU -- WPB in cc_fwd_bf16_kernel.h)
#define INV_VARIANT_W8(T, NR) { T, 1, NR, 2, 8, cc_fwd_bf16_kernel<T, 2, 1, true, NR, false, INV_MODE, 0, 8>, INV_KNAME "<T=" #T ",EXACT=1,LIVE=" #NR ",WAVES=8>" }
#define INV_VARIANT3(T, EX, NR) { T, EX, NR, 3, 4, cc_fwd_bf16_kernel<T, 3, 1, (EX) != 0, NR, false, INV_MODE>, INV_KNAME "<T=" #T ",PARTS=3,EXACT=" #EX ",LIVE=" #NR ">" }
// wide first hidden layer over a narrow rest (MNISTExperiment's integrand: sampling d = 784 images is 3 920 search launches)
struct InvWideFirst { int t1, nrl; inv_kernel_t fn; const char* name; };
#define INV_WIDE_FIRST(T, NR) { T, NR, cc_fwd_bf16_kernel<T, 2, 1, true, NR, false, INV_MODE, 4>, INV_KNAME "<T1=" #T ",TREST=4,LIVE=" #NR ">" }
static const InvWideFirst kInvWideFirst[] = { INV_WIDE_FIRST(5, 13), INV_WIDE_FIRST(6, 13), INV_WIDE_FIRST(7, 13), INV_WIDE_FIRST(8, 13),
                                              INV_WIDE_FIRST(5, 0), INV_WIDE_FIRST(6, 0), INV_WIDE_FIRST(7, 0), INV_WIDE_FIRST(8, 0) };
static const InvVariant kInvVariants[] = {
    INV_VARIANT(4, 1, 13), INV_VARIANT(4, 1, 0),       // UCI / VAE nets (31-50^4-1) and every other 3..4-tile net (zero-padded)
    INV_VARIANT(7, 1, 26), INV_VARIANT(7, 1, 0),       // 100-wide toy nets
    INV_VARIANT(5, 1, 0), INV_VARIANT(6, 1, 0), INV_VARIANT(8, 1, 0),
    INV_VARIANT_W8(7, 26), INV_VARIANT_W8(7, 0), INV_VARIANT_W8(5, 0), INV_VARIANT_W8(6, 0), INV_VARIANT_W8(8, 0),
    INV_VARIANT(2, 0, 0), INV_VARIANT(4, 0, 0), INV_VARIANT(8, 0, 0),   // generic (runtime tile counts): e.g. 20-20, mixed wide 70-90
#ifndef UMNN_FWD_PIECE_F16
    // three pieces / six cross terms (fwd_precision = fp32 | bf16x6): nets of up to four tiles per layer
    INV_VARIANT3(4, 1, 13), INV_VARIANT3(4, 1, 0), INV_VARIANT3(2, 0, 0), INV_VARIANT3(4, 0, 0),
#endif
};

// Which build and how many pieces for the library's fwd_precision.  f16x3 (default): two fp16 pieces (fp32-level products) with the
// queued bf16x3 fallback.  bf16x3: two bf16 pieces.  fp32 / bf16x6 ("exact products everywhere"): three bf16 pieces, which exist for
// up to four tiles per layer -- 8 tiles x 3 pieces do not fit the register file, so wider nets get their fp32-level products from
// the two-fp16-piece build instead: the same accuracy class, ~5e-7 on F; a tile whose integrals overflow fp16 is redone on two bf16
// pieces, ~6e-6 on F (for the search, orders of magnitude inside its own resolution 100 / 9^iter for all but the last rounds).
struct InvMode { bool f16; int nparts; };
inline InvMode inv_mode(int tmax) {
    const int prec = umnn_options().fwd_precision;
    if (prec == UMNN_PRECISION_F16X3 || (prec != UMNN_PRECISION_BF16X3 && tmax > 4)) return {true, 2};
    return {false, prec == UMNN_PRECISION_BF16X3 ? 2 : 3};
}

// What the search and the solve do not share.  The caller also fills the operand fields of a zeroed FwdBf16Args (NI, d, E, n included).
struct InvJob {
    const char* what;        // "invert" | "solve": prefix of the error texts, "cc_<what> launch"
    long long groups;        // tiles in the launch
    int scratch;             // floats of reduction scratch per wave when a tile's node range is split
    double flops;            // algorithmic work booked for the launch
};

// One launch.  ovf: bf16 build only -- non-null = the queued fallback of an fp16-piece launch.  queue_bf16(second) queues the
// two-piece bf16 build of the same job behind the launch of the fp16 build (overflow protocol: cc_forward_bf16.hip).
template <class QueueBf16>
static int inv_launch(const umnn_mlp* net, FwdBf16Args& args, const InvJob& job, int nparts, hipStream_t stream, const InvOvfPlan* ovf,
                      QueueBf16 queue_bf16) {
    FwdArgs& a = args.f;
    int tmax = 0, ksu = 0;
    if (int rc = umnn_prepare_mlp(net, a.E, &a.m, &tmax, &ksu)) return rc;
    const int L = a.m.n_linear - 1;
#ifdef UMNN_FWD_PIECE_F16
    InvOvfPlan own{1, nullptr, 0};
    if (int rc = umnn_ovf_slot(&own.flag, &own.gen)) return rc;
    ovf = &own;
#endif
    a.ovf_mode = ovf ? ovf->mode : 0; a.ovf_flag = ovf ? ovf->flag : nullptr; a.ovf_gen = ovf ? ovf->gen : 0;
    char msg[96];
    auto fail = [&](const char* text) { snprintf(msg, sizeof(msg), "%s: %s", job.what, text); return umnn_fail(UMNN_EUNSUPPORTED, msg); };
    // the planned launch: fp16 build = the launch, then the two-piece bf16 build of the same job queued as its fallback
    auto launch = [&](inv_kernel_t fn, const char* name, int wpb, size_t lds_bytes) -> int {
        if (int rc = umnn_allow_lds((const void*)fn, lds_bytes)) return rc;
        a.ngroups = (unsigned)job.groups;                  // one tile per wave, or per workgroup (small batches)
        const unsigned gpb = wpb / a.ns;
        const unsigned nblk = (a.ngroups + gpb - 1) / gpb;
        const bool queued = ovf && ovf->mode == 2;
        if (!queued) umnn_prof_begin(stream);
        hipLaunchKernelGGL(fn, dim3(nblk), dim3(64 * wpb), lds_bytes, stream, args);
        int rc = 0;
        if (const hipError_t e = hipGetLastError()) { snprintf(msg, sizeof(msg), "cc_%s launch", job.what); rc = umnn_check(e, msg); }
#ifdef UMNN_FWD_PIECE_F16
        const InvOvfPlan second{2, ovf->flag, ovf->gen};
        if (!rc) rc = queue_bf16(&second);
#else
        (void)queue_bf16;
#endif
        if (!queued) {
            umnn_prof_end(stream, job.flops);
            umnn_note_launch(name);
        }
        return rc;
    };
    // Small batches: one tile per WORKGROUP, its node range split over all the workgroup's waves (partials meet in LDS once per round
    // or iteration, in a fixed order) -- B waves of a 100-image sampling call leave nine SIMDs in ten idle, and every wave walks its
    // (n + 1) nodes alone.  Taken while all groups x wpb waves are resident at once (two per SIMD); the queued bf16 build gets the
    // same plan.
    auto split_over = [&](int wpb) -> int {
        return (job.groups * (long long)wpb <= (long long)umnn_num_cus() * 8 && wpb <= a.n + 1) ? wpb : 1;
    };
    a.ns = 1;
    FwdLayout lay;
    if (fwd_plan_wide_first(args, 2, &lay)) {                // (above four tiles every mode runs on two pieces: inv_mode)
        a.ns = split_over(UMNN_WAVES_PER_BLOCK);
        const size_t lds_bytes = ((size_t)a.m.lds_off[L] + (a.ns > 1 ? job.scratch * UMNN_WAVES_PER_BLOCK : 0)) * sizeof(float);
        const InvWideFirst* pick = nullptr;
        for (const InvWideFirst& v : kInvWideFirst) if (v.t1 == lay.T && v.nrl == lay.nrl) pick = &v;
        if (!pick || lds_bytes > 160 * 1024) return fail("weight images exceed 160 KiB of LDS");
        return launch(pick->fn, pick->name, UMNN_WAVES_PER_BLOCK, lds_bytes);
    }
    lay = fwd_plan_images(args, nparts, tmax, fwd_uniform_wide(a.m, tmax), true, 3);
    const size_t lds_bytes = (size_t)a.m.lds_off[L] * sizeof(float);
    if (lds_bytes > 160 * 1024) return fail("weight images exceed 160 KiB of LDS");
    // exact variant for (T, live registers) if instantiated, else the generic one of the tile-count bucket (runtime counts:
    // only reached by unpadded plans -- every padded or wide plan has its exact variant above)
    const int wpb = (lay.wide && lay.exact && nparts == 2 && 2 * (lds_bytes + 1024) > 160 * 1024) ? 8 : 4;      // one workgroup per CU: eight waves
    const InvVariant* pick = nullptr;
    for (int ex = lay.exact; ex >= 0 && !pick; --ex)
        for (int pass = 0; pass < 2 && !pick; ++pass)
            for (const InvVariant& v : kInvVariants)
                if (v.tmax == (ex ? lay.T : fwd_tile_bucket(tmax)) && v.exact == ex && v.nparts == nparts && v.wpb == (ex ? wpb : 4) &&
                    (pass == 0 ? (ex && lay.nrl && v.nrl == lay.nrl) : v.nrl == 0)) { pick = &v; break; }
    if (!pick) return fail("no kernel variant for this shape");
    a.ns = split_over(pick->wpb);
    size_t lds_run = lds_bytes + (a.ns > 1 ? (size_t)job.scratch * pick->wpb * sizeof(float) : 0);
    if (lds_run > 160 * 1024) { a.ns = 1; lds_run = lds_bytes; }
    return launch(pick->fn, pick->name, pick->wpb, lds_run);
}
