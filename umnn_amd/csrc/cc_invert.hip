// Sampling direction of a UMNNMAF block on the matrix cores: the reference's dimension-by-dimension bracket search
// (UMNNMAF.invert, models/UMNN/UMNNMAF.py:182-232, driven by UMNNMAFFlow.invert, UMNNMAFFlow.py:78-90) with the WHOLE search of
// one dimension -- `iter` rounds x 10 candidate integrals per sample -- inside one launch.  The reference issues, per
// dimension and round, a ParallelNeuralIntegral over [10*B, 1] rows (plus a MADE pass per dimension); here one dimension is
// the MADE pass + ONE launch of an INV variant of cc_fwd_bf16_kernel (cc_fwd_bf16_kernel.h): tile = sample, lane p = candidate
// p, the hoisted first-layer term computed once per sample, the argmin / new bracket a 16-lane butterfly between rounds.
// Arithmetic: bf16x3 split products in this build (F to ~6e-6 relative), orders of magnitude inside the search's own resolution:
// the bracket after k rounds is one candidate step wide, [cand_m, cand_m+1] or [cand_m-1, cand_m], i.e. 100 / 9^k.  A sample whose
// target or embedding is not a number returns NaN (its distances lose every comparison of the argmin: cc_fwd_bf16_kernel.h).
// Under fwd_precision = fp32 / bf16x6 ("the reference's arithmetic everywhere") nets of up to four tiles per layer run the same
// search with THREE bf16 pieces and six cross terms (PARTS=3: fp32-level products, ~4e-7 on F -- the matrix-core arithmetic of the
// bf16x6 forward mode; there is no fp32-MFMA form of this kernel); wider nets, whose three-piece form does not fit the register
// file (8 tiles x 3 pieces), run the two-fp16-piece search of the f16x3 mode instead (fwd_plan_inverse, cc_fwd_plan.h: the launch plan, shared with cc_solve.hip).
// This file is compiled twice, like cc_forward_bf16.hip: as is (bf16 pieces; exports umnn_flow_invert_dim) and through cc_invert_f16.hip
// with -DUMNN_FWD_PIECE_F16 (fp16 pieces: the search of the library's default arithmetic, f16x3).  The fp16 build follows the
// forward's overflow protocol (cc_fwd_launch.h): a sample for which any candidate integral of any round was not finite gets a NaN
// in its slot of x_inv[:, j] and raises the launch's flag word; the two-piece bf16 build of the same search, queued right behind it,
// returns at once when the flag is down and otherwise redoes exactly the samples whose slot holds the NaN.
#ifndef UMNN_ASM_TIED
#define UMNN_ASM_TIED 1      // cc_common.h: inline-assembly outputs tied to inputs in the forward translation units
#endif
#ifdef UMNN_FWD_PIECE_F16
#define INV_ROWS kInvertRowsF16
#define INV_IMPL umnn_invert_impl_f16
#else
#define INV_ROWS kInvertRowsBf16
#define INV_IMPL umnn_invert_impl_bf16
#endif
#define INV_MODE 1
#define INV_WHAT "invert"
#include "cc_inv_launch.h"
struct InvertCall {     // the operands of umnn_flow_invert_dim
    const float *h, *z, *scaling, *cc_w, *cc_s;
    int nb_steps;
    long long B;
    int d, E, j, iters;
    float* x_inv;
};
int umnn_invert_impl_bf16(const FwdPlan& pl, const InvertCall& c, double flops, hipStream_t stream, const UmnnOvfPlan* ovf);
int umnn_invert_impl_f16(const FwdPlan& pl, const InvertCall& c, double flops, hipStream_t stream, const UmnnOvfPlan* ovf);

// One launch of the search (see the file header): one tile (= one sample) per wave, or per workgroup.
int INV_IMPL(const FwdPlan& pl, const InvertCall& c, double flops, hipStream_t stream, const UmnnOvfPlan* ovf) {
    FwdBf16Args args{};
    FwdArgs& a = args.f;
    a.h = c.h; a.ccw = c.cc_w; a.ccs = c.cc_s; a.scaling = c.scaling;
    a.inv_z = c.z; a.inv_x = c.x_inv; a.inv_j = c.j; a.inv_iters = c.iters;
    a.NI = c.B; a.d = c.d; a.E = c.E; a.n = c.nb_steps;
    return inv_launch(pl, args, flops, stream, ovf,
                      [&](const UmnnOvfPlan& second) { return umnn_invert_impl_bf16(pl, c, flops, stream, &second); });
}

#ifndef UMNN_FWD_PIECE_F16
extern "C" int umnn_flow_invert_dim(const umnn_mlp* net, const float* h, const float* z, const float* scaling,
                                    const float* cc_w, const float* cc_s, int nb_steps,
                                    long long B, int d, int E, int j, int iters, float* x_inv, void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    if (!net) return umnn_fail(UMNN_EINVAL, "net is null");
    if (nb_steps < 1 || iters < 1) return umnn_fail(UMNN_EINVAL, "invert: nb_steps and iters must be >= 1");
    if (B < 0 || d < 1 || j < 0 || j >= d) return umnn_fail(UMNN_EINVAL, "invert: B >= 0, d >= 1, 0 <= j < d");
    MlpDev m; int tmax = 0, ksu = 0;
    if (int rc = umnn_prepare_mlp(net, E, &m, &tmax, &ksu)) return rc;
    if (B == 0) return 0;
    if (!h || !z || !scaling || !cc_w || !cc_s || !x_inv) return umnn_fail(UMNN_EINVAL, "invert: null pointer");
    // (build and pieces by fwd_precision -- never a silent ~6e-6 search under fp32 / bf16x6: fwd_plan_inverse)
    const FwdPlan pl = fwd_plan(m, tmax, ksu, fwd_call_search(B, nb_steps), umnn_fwd_options(), umnn_num_cus());
    if (pl.error) return umnn_fail(pl.error, pl.error_text);
    // algorithmic work: iters rounds x 10 candidate integrals per sample
    const double flops = umnn_cc_forward_flops_per_integral(net, nb_steps) * 10.0 * iters * (double)B;
    return (pl.f16 ? umnn_invert_impl_f16 : umnn_invert_impl_bf16)(pl, InvertCall{h, z, scaling, cc_w, cc_s, nb_steps, B, d, E, j, iters, x_inv},
                                                                  flops, stream, nullptr);
}
#endif
