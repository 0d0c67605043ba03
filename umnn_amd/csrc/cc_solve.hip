// Inverse of the monotone map G(x; h) = scale (off + int_0^x f(t; h) dt) on the matrix cores: a safeguarded Newton iteration with
// the WHOLE solve of one dimension inside one launch (umnn_cc_solve, include/umnn_cc.h).  Where the bracket search of cc_invert.hip
// spends 10 x iter quadratures per sample on a tile of its own, this uses what every quadrature already returns -- node 0 is x, so
// f(x) = dF/dx comes with F -- and converges in a handful of them, with the forward's layout: sixteen rows per tile, lane p = row
// 16 tile + p, each with its own iterate, bracket and done flag (the INV = 2 variants of cc_fwd_bf16_kernel.h).
// The variants, the launch plan (small batches: one tile per workgroup, where the partial sums and f(x) of the waves meet in LDS
// once per iteration in a fixed order, so every wave sees the same totals and takes the same branch -- 100 x 784 image sampling lives
// there) and the arithmetic modes are cc_fwd_plan.h's (fwd_plan_inverse), shared with the search: two fp16 pieces by default (this file compiled through
// cc_solve_f16.hip with -DUMNN_FWD_PIECE_F16), two bf16 pieces under bf16x3, three under fp32 / bf16x6 for nets of up to four tiles per
// layer.  Overflow protocol of the fp16 build: a row one of whose iterates produced a non-finite integral gets a NaN in its x slot and
// raises the launch's flag word; the two-piece bf16 build, queued right behind, returns at once when the flag is down and otherwise
// redoes the tiles that hold a NaN, writing only those rows.
// umnn_cc_solve_block runs the same launch over all B d (sample, dimension) pairs of a block under one embedding, optionally warm-started
// (one sweep of invert(method="jacobi")): the rows become the flat [B, d] index, everything else here is shared.
#ifndef UMNN_ASM_TIED
#define UMNN_ASM_TIED 1      // cc_common.h: inline-assembly outputs tied to inputs in the forward translation units
#endif
#ifdef UMNN_FWD_PIECE_F16
#define INV_ROWS kSolveRowsF16
#define INV_IMPL umnn_solve_impl_f16
#else
#define INV_ROWS kSolveRowsBf16
#define INV_IMPL umnn_solve_impl_bf16
#endif
#define INV_MODE 2
#define INV_WHAT "solve"
#include "cc_inv_launch.h"
struct SolveCall {      // the operands of umnn_cc_solve; umnn_cc_solve_block (block != 0): B = the B d flat rows, strides 1, j = 0
    const float *h, *target, *scale_row, *scaling, *off_row, *cc_w, *cc_s;
    long long t_stride, x_stride, B;
    int off_h0, nb_steps, d, E, j, max_iter;
    float lo, hi, tol;
    float *x, *f_x;
    int* status;
    int block;
    const float* x_init;
    float* lj_row = nullptr;     // umnn_cc_solve_lj: the rows' running log-Jacobian (SolveArgs::lj_row), null otherwise
    int lj_first = 0;
};
int umnn_solve_impl_bf16(const FwdPlan& pl, const SolveCall& c, double flops, hipStream_t stream, const UmnnOvfPlan* ovf);
int umnn_solve_impl_f16(const FwdPlan& pl, const SolveCall& c, double flops, hipStream_t stream, const UmnnOvfPlan* ovf);

// One launch of the solve (see the file header): one tile (sixteen rows) per wave, or per workgroup.
int INV_IMPL(const FwdPlan& pl, const SolveCall& c, double flops, hipStream_t stream, const UmnnOvfPlan* ovf) {
    FwdBf16Args args{};
    FwdArgs& a = args.f;
    a.x = c.x_init; a.h = c.h; a.ccw = c.cc_w; a.ccs = c.cc_s; a.fx = c.f_x; a.scaling = c.scaling;
    a.inv_z = c.target; a.inv_x = c.x; a.inv_j = c.j; a.inv_iters = c.max_iter;
    args.sv.t_stride = c.t_stride; args.sv.x_stride = c.x_stride; args.sv.scale_row = c.scale_row; args.sv.off_row = c.off_row;
    args.sv.off_h0 = c.off_h0; args.sv.status = c.status; args.sv.lo = c.lo; args.sv.hi = c.hi; args.sv.tol = c.tol;
    args.sv.block = c.block; args.sv.lj_row = c.lj_row; args.sv.lj_first = c.lj_first;
    a.NI = c.B; a.d = c.d; a.E = c.E; a.n = c.nb_steps;
    return inv_launch(pl, args, flops, stream, ovf, [&](const UmnnOvfPlan& second) { return umnn_solve_impl_bf16(pl, c, flops, stream, &second); });
}

#ifndef UMNN_FWD_PIECE_F16
// Validation and launch plan (build and pieces by fwd_precision: fwd_plan_inverse) of both entry points.
static int solve_entry(const umnn_mlp* net, const SolveCall& c, hipStream_t stream) {
    if (!net) return umnn_fail(UMNN_EINVAL, "net is null");
    if (c.nb_steps < 1 || c.max_iter < 1 || c.max_iter > UMNN_SOLVE_EVALS_MASK)
        return umnn_fail(UMNN_EINVAL, "solve: nb_steps >= 1 and 1 <= max_iter <= 65535");
    if (c.B < 0 || c.d < 1 || c.j < 0 || c.j >= c.d)
        return umnn_fail(UMNN_EINVAL, c.block ? "solve: B >= 0, d >= 1" : "solve: B >= 0, d >= 1, 0 <= j < d");
    if (!(c.lo < c.hi) || !(c.tol >= 0.f)) return umnn_fail(UMNN_EINVAL, "solve: lo < hi and tol >= 0");
    if (c.t_stride <= c.j || c.x_stride <= c.j) return umnn_fail(UMNN_EINVAL, "solve: row strides must exceed j");
    MlpDev m; int tmax = 0, ksu = 0;
    if (int rc = umnn_prepare_mlp(net, c.E, &m, &tmax, &ksu)) return rc;
    if (c.B == 0) return 0;
    if (!c.h || !c.target || !c.cc_w || !c.cc_s || !c.x) return umnn_fail(UMNN_EINVAL, "solve: null pointer");
    const FwdPlan pl = fwd_plan(m, tmax, ksu, fwd_call_solve(c.B, c.nb_steps), umnn_fwd_options(), umnn_num_cus());
    if (pl.error) return umnn_fail(pl.error, pl.error_text);
    // algorithmic work: the iteration count is decided inside the launch -- booked at four quadratures per row, the typical count
    const double flops = umnn_cc_forward_flops_per_integral(net, c.nb_steps) * 4.0 * (double)c.B;
    return (pl.f16 ? umnn_solve_impl_f16 : umnn_solve_impl_bf16)(pl, c, flops, stream, nullptr);
}

extern "C" int umnn_cc_solve(const umnn_mlp* net, const float* h, const float* target, long long t_stride,
                             const float* scale_row, const float* scaling, const float* off_row, int off_h0,
                             const float* cc_w, const float* cc_s, int nb_steps, long long B, int d, int E, int j,
                             float lo, float hi, float tol, int max_iter,
                             float* x, long long x_stride, float* f_x, int* status, void* stream_) {
    return solve_entry(net, SolveCall{h, target, scale_row, scaling, off_row, cc_w, cc_s, t_stride, x_stride, B, off_h0, nb_steps, d, E, j,
                                      max_iter, lo, hi, tol, x, f_x, status, 0, nullptr}, (hipStream_t)stream_);
}

// umnn_cc_solve that also adds the row's log-Jacobian at the returned x to lj_row (include/umnn_cc.h): the same launch, plan and kernel.
extern "C" int umnn_cc_solve_lj(const umnn_mlp* net, const float* h, const float* target, long long t_stride,
                                const float* scale_row, const float* scaling, const float* off_row, int off_h0,
                                const float* cc_w, const float* cc_s, int nb_steps, long long B, int d, int E, int j,
                                float lo, float hi, float tol, int max_iter,
                                float* x, long long x_stride, float* f_x, int* status, float* lj_row, int lj_first, void* stream_) {
    if (lj_first != 0 && lj_first != 1) return umnn_fail(UMNN_EINVAL, "solve: lj_first is 0 or 1");
    SolveCall c{h, target, scale_row, scaling, off_row, cc_w, cc_s, t_stride, x_stride, B, off_h0, nb_steps, d, E, j,
                max_iter, lo, hi, tol, x, f_x, status, 0, nullptr};
    c.lj_row = lj_row; c.lj_first = lj_first;
    return solve_entry(net, c, (hipStream_t)stream_);
}

// The same solve for every (row, dimension) of a block in ONE launch (include/umnn_cc.h): the rows of the launch are the flat index
// q = b d + i over [B, d], sixteen to a tile as in the forward kernels (strides 1 and j = 0 pass the row checks of solve_entry).
extern "C" int umnn_cc_solve_block(const umnn_mlp* net, const float* h, const float* target, const float* scaling, int off_h0,
                                   const float* x_init, const float* cc_w, const float* cc_s, int nb_steps,
                                   long long B, int d, int E, float lo, float hi, float tol, int max_iter,
                                   float* x, float* f_x, int* status, void* stream_) {
    const long long rows = d < 1 ? B : B * (long long)d;
    return solve_entry(net, SolveCall{h, target, nullptr, scaling, nullptr, cc_w, cc_s, 1, 1, rows, off_h0, nb_steps, d, E, 0, max_iter,
                                      lo, hi, tol, x, f_x, status, 1, x_init}, (hipStream_t)stream_);
}
#endif
