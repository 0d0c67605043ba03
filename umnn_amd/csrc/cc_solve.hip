// Inverse of the monotone map G(x; h) = scale (off + int_0^x f(t; h) dt) on the matrix cores: a safeguarded Newton iteration with
// the WHOLE solve of one dimension inside one launch (umnn_cc_solve, include/umnn_cc.h).  Where the bracket search of cc_invert.hip
// spends 10 x iter quadratures per sample on a tile of its own, this uses what every quadrature already returns -- node 0 is x, so
// f(x) = dF/dx comes with F -- and converges in a handful of them, with the forward's layout: sixteen rows per tile, lane p = row
// 16 tile + p, each with its own iterate, bracket and done flag (the INV = 2 variants of cc_fwd_bf16_kernel.h).
// The variant tables, the launch plan and the arithmetic modes are those of cc_invert.hip: two fp16 pieces by default (this file
// compiled through cc_solve_f16.hip with -DUMNN_FWD_PIECE_F16), two bf16 pieces under bf16x3, three under fp32 / bf16x6 for nets of up
// to four tiles per layer.  Overflow protocol of the fp16 build: a row one of whose iterates produced a non-finite integral gets a NaN
// in its x slot and raises the launch's flag word; the two-piece bf16 build, queued right behind, returns at once when the flag is down
// and otherwise redoes the tiles that hold a NaN, writing only those rows.
// Small batches: one tile per WORKGROUP, its node range split over the workgroup's waves; partial sums and f(x) meet in LDS once per
// iteration in a fixed order, so every wave sees the same totals and takes the same branch (100 x 784 image sampling lives here).
// umnn_cc_solve_block runs the same launch over all B d (sample, dimension) pairs of a block under one embedding, optionally warm-started
// (one sweep of invert(method="jacobi")): the rows become the flat [B, d] index, everything else here is shared.
#ifndef UMNN_ASM_TIED
#define UMNN_ASM_TIED 1      // cc_common.h: inline-assembly outputs tied to inputs in the forward translation units
#endif
#include "cc_fwd_bf16_kernel.h"
using namespace UMNN_FWD_NS;
#ifdef UMNN_FWD_PIECE_F16
#define INV_KNAME "cc_solve_f16"
#define INV_IMPL umnn_solve_impl_f16
#else
#define INV_KNAME "cc_solve_bf16"
#define INV_IMPL umnn_solve_impl_bf16
#endif
struct InvOvfPlan { int mode; unsigned long long* flag; unsigned long long gen; };
int umnn_ovf_slot(unsigned long long** flag, unsigned long long* gen);                                  // cc_api.hip
struct SolveCall {      // the operands of umnn_cc_solve; umnn_cc_solve_block (block != 0): B = the B d flat rows, strides 1, j = 0
    const float *h, *target, *scale_row, *scaling, *off_row, *cc_w, *cc_s;
    long long t_stride, x_stride, B;
    int off_h0, nb_steps, d, E, j, max_iter;
    float lo, hi, tol;
    float *x, *f_x;
    int* status;
    int block;
    const float* x_init;
};
int umnn_solve_impl_bf16(const umnn_mlp* net, const SolveCall& c, hipStream_t stream, int nparts, const InvOvfPlan* ovf);
int umnn_solve_impl_f16(const umnn_mlp* net, const SolveCall& c, hipStream_t stream, int nparts, const InvOvfPlan* ovf);

typedef void (*inv_kernel_t)(const FwdBf16Args);
struct InvVariant { int tmax, exact, nrl, nparts, wpb; inv_kernel_t fn; const char* name; };
#define INV_VARIANT(T, EX, NR) { T, EX, NR, 2, 4, cc_fwd_bf16_kernel<T, 2, 1, (EX) != 0, NR, false, 2>, INV_KNAME "<T=" #T ",EXACT=" #EX ",LIVE=" #NR ">" }
// (eight waves per workgroup: images that leave room for one workgroup per CU -- WPB in cc_fwd_bf16_kernel.h)
#define INV_VARIANT_W8(T, NR) { T, 1, NR, 2, 8, cc_fwd_bf16_kernel<T, 2, 1, true, NR, false, 2, 0, 8>, INV_KNAME "<T=" #T ",EXACT=1,LIVE=" #NR ",WAVES=8>" }
#define INV_VARIANT3(T, EX, NR) { T, EX, NR, 3, 4, cc_fwd_bf16_kernel<T, 3, 1, (EX) != 0, NR, false, 2>, INV_KNAME "<T=" #T ",PARTS=3,EXACT=" #EX ",LIVE=" #NR ">" }
// wide first hidden layer over a narrow rest (MNISTExperiment's integrand: sampling d = 784 images is 3 920 of these launches)
struct InvWideFirst { int t1, nrl; inv_kernel_t fn; const char* name; };
#define INV_WIDE_FIRST(T, NR) { T, NR, cc_fwd_bf16_kernel<T, 2, 1, true, NR, false, 2, 4>, INV_KNAME "<T1=" #T ",TREST=4,LIVE=" #NR ">" }
static const InvWideFirst kInvWideFirst[] = { INV_WIDE_FIRST(5, 13), INV_WIDE_FIRST(6, 13), INV_WIDE_FIRST(7, 13), INV_WIDE_FIRST(8, 13),
                                              INV_WIDE_FIRST(5, 0), INV_WIDE_FIRST(6, 0), INV_WIDE_FIRST(7, 0), INV_WIDE_FIRST(8, 0) };
static const InvVariant kInvVariants[] = {
    INV_VARIANT(4, 1, 13), INV_VARIANT(4, 1, 0),       // UCI / VAE nets (31-50^4-1) and every other 3..4-tile net (zero-padded)
    INV_VARIANT(7, 1, 26), INV_VARIANT(7, 1, 0),       // 100-wide toy nets
    INV_VARIANT(5, 1, 0), INV_VARIANT(6, 1, 0), INV_VARIANT(8, 1, 0),
    INV_VARIANT_W8(7, 26), INV_VARIANT_W8(7, 0), INV_VARIANT_W8(5, 0), INV_VARIANT_W8(6, 0), INV_VARIANT_W8(8, 0),
    INV_VARIANT(2, 0, 0), INV_VARIANT(4, 0, 0), INV_VARIANT(8, 0, 0),   // generic (runtime tile counts): mixed widths, e.g. 100-50-50-50-50
#ifndef UMNN_FWD_PIECE_F16
    // three pieces / six cross terms (fwd_precision = fp32 | bf16x6): nets of up to four tiles per layer
    INV_VARIANT3(4, 1, 13), INV_VARIANT3(4, 1, 0), INV_VARIANT3(2, 0, 0), INV_VARIANT3(4, 0, 0),
#endif
};

// One launch of the solve (see the file header); ovf: bf16 build only -- non-null = the queued fallback of an fp16-piece launch.
int INV_IMPL(const umnn_mlp* net, const SolveCall& c, hipStream_t stream, int nparts, const InvOvfPlan* ovf) {
    const int E = c.E, d = c.d, nb_steps = c.nb_steps;
    const long long B = c.B, ntiles = (c.B + 15) / 16;
    FwdBf16Args args;
    FwdArgs& a = args.f;
    int tmax = 0, ksu = 0;
    if (int rc = umnn_prepare_mlp(net, E, &a.m, &tmax, &ksu)) return rc;
    const int L = a.m.n_linear - 1;
#ifdef UMNN_FWD_PIECE_F16
    InvOvfPlan own{1, nullptr, 0};
    if (int rc = umnn_ovf_slot(&own.flag, &own.gen)) return rc;
    ovf = &own;
#endif
    a.ovf_mode = ovf ? ovf->mode : 0; a.ovf_flag = ovf ? ovf->flag : nullptr; a.ovf_gen = ovf ? ovf->gen : 0;
    // the planned launch: fp16 build = the launch, then the two-piece bf16 build of the same search queued as its fallback
    auto launch = [&](inv_kernel_t fn, const char* name, unsigned nblk, size_t lds_bytes, int block = UMNN_BLOCK) -> int {
        const bool queued = ovf && ovf->mode == 2;
        if (!queued) umnn_prof_begin(stream);
        hipLaunchKernelGGL(fn, dim3(nblk), dim3(block), lds_bytes, stream, args);
        int rc = umnn_check(hipGetLastError(), "cc_solve launch");
#ifdef UMNN_FWD_PIECE_F16
        const InvOvfPlan second{2, ovf->flag, ovf->gen};
        if (!rc) rc = umnn_solve_impl_bf16(net, c, stream, 2, &second);
#endif
        if (!queued) {
            // algorithmic work: the iteration count is decided inside the launch -- booked at four quadratures per row, the typical count
            umnn_prof_end(stream, umnn_cc_forward_flops_per_integral(net, nb_steps) * 4.0 * (double)B);
            umnn_note_launch(name);
        }
        return rc;
    };
    // Small batches: one tile per WORKGROUP, its node range split over all the workgroup's waves (partials meet in LDS once per
    // iteration).  Taken while all tiles x wpb waves are resident at once (two per SIMD); the queued bf16 build gets the same plan.
    auto split_over = [&](int wpb) -> int {
        return (ntiles * (long long)wpb <= (long long)umnn_num_cus() * 8 && wpb <= nb_steps + 1) ? wpb : 1;
    };
    a.x0 = nullptr; a.x = c.x_init; a.h = c.h; a.ccw = c.cc_w; a.ccs = c.cc_s;
    a.F = a.fx0 = nullptr; a.fx = c.f_x; a.scaling = c.scaling; a.z = nullptr; a.logjac = nullptr; a.logjac_in = nullptr;
    a.reverse_z = 0; a.ll = nullptr; a.row_cnt = nullptr; a.ll_first = a.ll_last = 0;
    a.inv_z = c.target; a.inv_x = c.x; a.inv_j = c.j; a.inv_iters = c.max_iter;
    args.sv.t_stride = c.t_stride; args.sv.x_stride = c.x_stride; args.sv.scale_row = c.scale_row; args.sv.off_row = c.off_row;
    args.sv.off_h0 = c.off_h0; args.sv.status = c.status; args.sv.lo = c.lo; args.sv.hi = c.hi; args.sv.tol = c.tol;
    args.sv.block = c.block;
    a.NI = B; a.d = d; a.E = E; a.n = nb_steps; a.inv_f = 0; a.ns = 1; a.x_bf16 = 0; a.h_bf16 = 0; a.z2_save = nullptr; a.z2_nl2 = 0;

    // ---- wide first hidden layer, every other layer at most four tiles: shape-exact family (as in cc_forward_bf16.hip)
    {
        bool wf = a.m.t_out[1] >= 5 && a.m.t_out[1] <= 8;
        for (int l = 2; l <= L && wf; ++l) if (a.m.t_out[l] > 4) wf = false;
        if (wf) {
            const int T1 = a.m.t_out[1];
            int o16 = 0;
            for (int l = 1; l <= L; ++l) {
                args.pl.ks32[l] = l == 1 ? T1 / 2 : 2;
                args.pl.half_in[l] = l == 1 ? (T1 & 1) : 0;
                if (l >= 2) a.m.t_out[l] = 4;
            }
            for (int l = 1; l < L; ++l) {
                args.pl.off16[l] = o16;
                o16 += 4 * (args.pl.ks32[l] * 2 * 512 + args.pl.half_in[l] * 2 * 256);
            }
            a.m.lds_off[L] = (((o16 + 1) / 2) + 3) & ~3;
            a.ns = split_over(UMNN_WAVES_PER_BLOCK);
            const size_t lds_bytes = ((size_t)a.m.lds_off[L] + (a.ns > 1 ? 2 * UMNN_WAVES_PER_BLOCK * 16 : 0)) * sizeof(float);
            int nrest = a.m.ks_in[2];           // live registers of the later layers when they all agree (13 = widths 48..51)
            for (int l = 2; l <= L; ++l) if (a.m.ks_in[l] != nrest) nrest = 0;
            if (nrest != 13) nrest = 0;
            const InvWideFirst* pick = nullptr;
            for (const InvWideFirst& v : kInvWideFirst) if (v.t1 == T1 && v.nrl == nrest) pick = &v;
            if (pick && lds_bytes <= 160 * 1024) {
                if (int rc = umnn_allow_lds((const void*)pick->fn, lds_bytes)) return rc;
                a.ngroups = (unsigned)ntiles;
                const unsigned gpb = UMNN_WAVES_PER_BLOCK / a.ns;
                const unsigned nblk = (a.ngroups + gpb - 1) / gpb;
                return launch(pick->fn, pick->name, nblk, lds_bytes);
            }
            return umnn_fail(UMNN_EUNSUPPORTED, "solve: weight images exceed 160 KiB of LDS");
        }
    }
    // ---- plan (the P = 1, two-piece subset of umnn_launch_forward_bf16's) ----
    int T = tmax <= 2 ? 2 : tmax <= 4 ? 4 : 8;
    int wide = tmax >= 5 ? tmax : 0;
    for (int l = 1; l <= L && wide; ++l) if (a.m.t_out[l] != wide) wide = 0;
    if (wide) T = wide;
    int off16 = 0;
    for (int l = 1; l <= L; ++l) {
        args.pl.half_in[l] = wide ? (wide & 1) : 0;
        args.pl.ks32[l] = wide ? wide / 2 : (a.m.t_out[l] + 1) / 2;
    }
    for (int l = 1; l < L; ++l) {
        args.pl.off16[l] = off16;
        off16 += a.m.t_out[l + 1] * (args.pl.ks32[l] * nparts * 512 + args.pl.half_in[l] * nparts * 256);
    }
    int exact = 1, nrl = a.m.ks_in[1];
    for (int l = 1; l <= L; ++l) {
        exact = exact && a.m.t_out[l] == T;
        if (a.m.ks_in[l] != nrl) nrl = 0;
    }
    if (!exact && !wide && tmax <= 4 && tmax >= 3) {       // mixed 3..4-tile nets: zero-pad to the shape-exact kernel
        T = 4; exact = 1; nrl = 0;
        for (int l = 1; l <= L; ++l) { a.m.t_out[l] = 4; args.pl.ks32[l] = 2; }
        off16 = 0;
        for (int l = 1; l < L; ++l) { args.pl.off16[l] = off16; off16 += 4 * 2 * nparts * 512; }
    }
    a.m.lds_off[L] = (((off16 + 1) / 2) + 3) & ~3;
    const size_t lds_bytes = (size_t)a.m.lds_off[L] * sizeof(float);
    if (lds_bytes > 160 * 1024) return umnn_fail(UMNN_EUNSUPPORTED, "solve: weight images exceed 160 KiB of LDS");
    // exact variant for (T, live registers) if instantiated, else the generic one of the tile-count bucket (runtime counts:
    // only reached by unpadded plans -- every padded or wide plan has its exact variant above)
    const int wpb = (wide && exact && nparts == 2 && 2 * (lds_bytes + 1024) > 160 * 1024) ? 8 : 4;      // one workgroup per CU: eight waves
    const InvVariant* pick = nullptr;
    for (int ex = exact; ex >= 0 && !pick; --ex)
        for (int pass = 0; pass < 2 && !pick; ++pass)
            for (const InvVariant& v : kInvVariants)
                if (v.tmax == (ex ? T : (tmax <= 2 ? 2 : tmax <= 4 ? 4 : 8)) && v.exact == ex && v.nparts == nparts && v.wpb == (ex ? wpb : 4) &&
                    (pass == 0 ? (ex && nrl && v.nrl == nrl) : v.nrl == 0)) { pick = &v; break; }
    if (!pick) return umnn_fail(UMNN_EUNSUPPORTED, "solve: no kernel variant for this shape");
    a.ngroups = (unsigned)ntiles;                                  // one tile (sixteen rows) per wave, or per workgroup (small batches)
    a.ns = split_over(pick->wpb);
    size_t lds_run = lds_bytes + (a.ns > 1 ? (size_t)2 * pick->wpb * 16 * sizeof(float) : 0);
    if (lds_run > 160 * 1024) { a.ns = 1; lds_run = lds_bytes; }
    if (int rc = umnn_allow_lds((const void*)pick->fn, lds_run)) return rc;
    const unsigned gpb = pick->wpb / a.ns;
    const unsigned nblk = (a.ngroups + gpb - 1) / gpb;
    return launch(pick->fn, pick->name, nblk, lds_run, 64 * pick->wpb);
}

#ifndef UMNN_FWD_PIECE_F16
extern "C" int umnn_cc_solve(const umnn_mlp* net, const float* h, const float* target, long long t_stride,
                             const float* scale_row, const float* scaling, const float* off_row, int off_h0,
                             const float* cc_w, const float* cc_s, int nb_steps, long long B, int d, int E, int j,
                             float lo, float hi, float tol, int max_iter,
                             float* x, long long x_stride, float* f_x, int* status, void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    if (!net) return umnn_fail(UMNN_EINVAL, "net is null");
    if (nb_steps < 1 || max_iter < 1 || max_iter > UMNN_SOLVE_EVALS_MASK)
        return umnn_fail(UMNN_EINVAL, "solve: nb_steps >= 1 and 1 <= max_iter <= 65535");
    if (B < 0 || d < 1 || j < 0 || j >= d) return umnn_fail(UMNN_EINVAL, "solve: B >= 0, d >= 1, 0 <= j < d");
    if (!(lo < hi) || !(tol >= 0.f)) return umnn_fail(UMNN_EINVAL, "solve: lo < hi and tol >= 0");
    if (t_stride <= j || x_stride <= j) return umnn_fail(UMNN_EINVAL, "solve: row strides must exceed j");
    MlpDev m; int tmax = 0, ksu = 0;
    if (int rc = umnn_prepare_mlp(net, E, &m, &tmax, &ksu)) return rc;
    if (B == 0) return 0;
    if (!h || !target || !cc_w || !cc_s || !x) return umnn_fail(UMNN_EINVAL, "solve: null pointer");
    if (m.n_linear - 1 < 2) return umnn_fail(UMNN_EUNSUPPORTED, "solve: the matrix-core kernels need at least two hidden layers");
    const SolveCall c{h, target, scale_row, scaling, off_row, cc_w, cc_s, t_stride, x_stride, B, off_h0, nb_steps, d, E, j, max_iter,
                      lo, hi, tol, x, f_x, status, 0, nullptr};
    // arithmetic modes as in umnn_flow_invert_dim (cc_invert.hip): f16x3 = two fp16 pieces with the queued bf16x3 fallback; bf16x3 = two
    // bf16 pieces; fp32 / bf16x6 = three bf16 pieces up to four tiles per layer, two fp16 pieces (the same accuracy class) above
    const int prec = umnn_options().fwd_precision;
    if (prec == UMNN_PRECISION_F16X3) return umnn_solve_impl_f16(net, c, stream, 2, nullptr);
    const int nparts = prec == UMNN_PRECISION_BF16X3 ? 2 : 3;
    if (nparts == 3 && tmax > 4) return umnn_solve_impl_f16(net, c, stream, 2, nullptr);
    return umnn_solve_impl_bf16(net, c, stream, nparts, nullptr);
}

// The same solve for every (row, dimension) of a block in ONE launch (include/umnn_cc.h): the rows of the launch are the flat index
// q = b d + i over [B, d], sixteen to a tile as in the forward kernels; everything else -- variants, plans, modes -- is umnn_cc_solve's.
extern "C" int umnn_cc_solve_block(const umnn_mlp* net, const float* h, const float* target, const float* scaling, int off_h0,
                                   const float* x_init, const float* cc_w, const float* cc_s, int nb_steps,
                                   long long B, int d, int E, float lo, float hi, float tol, int max_iter,
                                   float* x, float* f_x, int* status, void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    if (!net) return umnn_fail(UMNN_EINVAL, "net is null");
    if (nb_steps < 1 || max_iter < 1 || max_iter > UMNN_SOLVE_EVALS_MASK)
        return umnn_fail(UMNN_EINVAL, "solve: nb_steps >= 1 and 1 <= max_iter <= 65535");
    if (B < 0 || d < 1) return umnn_fail(UMNN_EINVAL, "solve: B >= 0, d >= 1");
    if (!(lo < hi) || !(tol >= 0.f)) return umnn_fail(UMNN_EINVAL, "solve: lo < hi and tol >= 0");
    MlpDev m; int tmax = 0, ksu = 0;
    if (int rc = umnn_prepare_mlp(net, E, &m, &tmax, &ksu)) return rc;
    if (B == 0) return 0;
    if (!h || !target || !cc_w || !cc_s || !x) return umnn_fail(UMNN_EINVAL, "solve: null pointer");
    if (m.n_linear - 1 < 2) return umnn_fail(UMNN_EUNSUPPORTED, "solve: the matrix-core kernels need at least two hidden layers");
    const SolveCall c{h, target, nullptr, scaling, nullptr, cc_w, cc_s, 1, 1, B * (long long)d, off_h0, nb_steps, d, E, 0, max_iter,
                      lo, hi, tol, x, f_x, status, 1, x_init};
    const int prec = umnn_options().fwd_precision;                 // (modes as in umnn_cc_solve)
    if (prec == UMNN_PRECISION_F16X3) return umnn_solve_impl_f16(net, c, stream, 2, nullptr);
    const int nparts = prec == UMNN_PRECISION_BF16X3 ? 2 : 3;
    if (nparts == 3 && tmax > 4) return umnn_solve_impl_f16(net, c, stream, 2, nullptr);
    return umnn_solve_impl_bf16(net, c, stream, nparts, nullptr);
}
#endif
