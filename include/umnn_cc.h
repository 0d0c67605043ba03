/*
 * umnn_cc.h -- C ABI of the MI355X (gfx950) Clenshaw-Curtis neural-integration library.
 *
 * The reference (AWehenkel/UMNN, pure Python) has no FFI; its operator boundary for this
 * path is the Python call
 *
 *     ParallelNeuralIntegral.apply(x0, x, integrand, flat_params, h, nb_steps, inv_f)
 *         models/UMNN/ParallelNeuralIntegral.py:97-123   (forward :100-108, backward :110-123)
 *     NeuralIntegral.apply(x0, x, integrand, flat_params, h, nb_steps)
 *         models/UMNN/NeuralIntegral.py:78-99
 *     integrate(x0, nb_steps, step_sizes, integrand, h, compute_grad, x_tot, inv_f, cc_weights, steps)
 *         models/UMNN/ParallelNeuralIntegral.py:37-80,  models/UMNN/NeuralIntegral.py:37-66
 *     compute_cc_weights(nb_steps)
 *         models/UMNN/ParallelNeuralIntegral.py:14-34
 *
 * and, one level up, the per-block flow arithmetic of models/UMNN/UMNNMAF.py:76-139
 * (z = exp(scaling) * (integral + h[:,0,:]),  log_jac = log(f(x;h) + 1e-10) + scaling).
 *
 * Each entry point below replaces one of those calls when the integrand is an MLP
 * (models/UMNN/UMNNMAF.py:235-284 IntegrandNetwork, models/UMNN/MonotonicNN.py:12-27
 * IntegrandNN).  Plain pointers and sizes only: every pointer is a DEVICE pointer to fp32
 * data owned by the caller (PyTorch's caching allocator in the shipped host code) unless the
 * name ends in _host.  Work is enqueued on `stream` (a hipStream_t passed as void*; NULL =
 * the default stream) and the call returns without synchronising.
 *
 * Layouts (identical to the reference tensors, contiguous, row-major):
 *     x0, x, F, f_x, f_x0, g, dx, dx0, z, log_jac   [B, d]
 *     h, dh                                         [B, E*d], element (b, e*d + i)  (UMNNMAF.py:279-281)
 *     W[l]  [widths[l+1], widths[l]]   b[l]  [widths[l+1]]     (torch.nn.Linear layout)
 *     cc_w, cc_s                                    [nb_steps+1]
 *
 * Return value: 0 on success, otherwise a negative UMNN_E* code or a positive hipError_t;
 * umnn_last_error() gives the message (thread-local).
 */
#ifndef UMNN_CC_H
#define UMNN_CC_H

#ifdef __cplusplus
extern "C" {
#endif

#define UMNN_MAX_LINEAR 8            /* Linear layers in the integrand MLP (hidden layers + 1) */
#define UMNN_MAX_HIDDEN_WIDTH 127    /* widest hidden layer the LDS-resident kernels accept */
#define UMNN_MAX_OUTPUTS 16          /* widest output layer of the multi-output entry points (umnn_cc_forward_multi) */

#define UMNN_ACT_LEAKY_RELU 0        /* nn.LeakyReLU(0.01): IntegrandNetwork, UMNNMAF.py:247 */
#define UMNN_ACT_RELU 1              /* nn.ReLU: IntegrandNN, MonotonicNN.py:20 */
#define UMNN_OUT_ELU_PLUS_ONE 0      /* ELU(.)+1: ELUPlus UMNNMAF.py:11-16 / MonotonicNN.py:23,27 */
#define UMNN_OUT_SIGMOID 1           /* nn.Sigmoid: dict_act_func UMNNMAF.py:19 */

#define UMNN_EINVAL (-1)             /* bad argument (message says which) */
#define UMNN_EUNSUPPORTED (-2)       /* shape outside what the kernels cover */
#define UMNN_ENODEVICE (-3)          /* no gfx950 device / kernel image not loadable */

typedef struct umnn_mlp {
    int n_linear;                         /* number of Linear layers */
    int widths[UMNN_MAX_LINEAR + 1];      /* [1+E, H1, ..., HL, 1]  (last entry K = 2..UMNN_MAX_OUTPUTS for the *_multi entry points only) */
    const float* W[UMNN_MAX_LINEAR];      /* device pointers */
    const float* b[UMNN_MAX_LINEAR];
    int hidden_act;                       /* UMNN_ACT_* */
    int out_act;                          /* UMNN_OUT_* */
} umnn_mlp;

/* Storage types of the activation tensors (configuration C4, the bf16 VAE prior flow: models/vae_lib/models/flows.py:305-323).
 * The arithmetic is fp32 in every case; the *_io entry points take a descriptor saying how the caller STORES
 *   x-class tensors: x0, x, F, f_x, f_x0, z, log_jac, log_jac_in, g, g_fx, dx, dx0      (x_dtype)
 *   h-class tensors: h (the [B, E*d] embedding the conditioner writes -- the large one), dh   (h_dtype)
 * bf16 loads are exact widenings, bf16 stores round to nearest even.  io == NULL means fp32 everywhere (= the plain
 * entry points).  d_theta, the quadrature tables, scaling and the weights are always fp32. */
#define UMNN_DTYPE_F32 0
#define UMNN_DTYPE_BF16 1
typedef struct umnn_io {
    int x_dtype;
    int h_dtype;
} umnn_io;

/* Replaces integrate(..., compute_grad=False) -- ParallelNeuralIntegral.py:49-65 and
 * NeuralIntegral.py:53-66 (both solvers are the same arithmetic; the kernel never
 * materialises the node axis).  Quadrature node 0 is x and node n is x0, so the same pass
 * also yields f(x;h) and f(x0;h) (what backward's Leibniz terms :117-118 and
 * UMNNMAF.compute_log_jac :138 re-evaluate in the reference).
 *   x0     may be NULL (= zeros, the only value UMNNMAF/MonotonicNN ever pass)
 *   inv_f  != 0 integrates 1/f (ParallelNeuralIntegral.py:58-59)
 *   f_x, f_x0 may be NULL. */
int umnn_cc_forward(const umnn_mlp* net, const float* x0, const float* x, const float* h,
                    const float* cc_w, const float* cc_s, int nb_steps,
                    long long B, int d, int E, int inv_f,
                    float* F, float* f_x, float* f_x0, void* stream);

/* Replaces one UMNNMAF block's arithmetic after the conditioner (UMNNMAF.py:80-83,134,138-139):
 *   z = exp(scaling_i) * (int_0^x f + h[b, 0*d+i]),  log_jac = log(f(x;h) + 1e-10) + scaling_i.
 * f_x / f_x0 (nullable) are also written so the autograd wrapper need not recompute them. */
int umnn_flow_block_forward(const umnn_mlp* net, const float* x, const float* h, const float* scaling,
                            const float* cc_w, const float* cc_s, int nb_steps,
                            long long B, int d, int E,
                            float* z, float* log_jac, float* f_x, float* f_x0, void* stream);

/* The same block as one link of a UMNNMAFFlow stack (UMNNMAFFlow.py:109-123: `for net: z, lj = ...; log_jac += lj;
 * x = z[:, inv_idx]`), with the glue between blocks folded into the kernel's stores:
 *   reverse_z != 0   z is written with its dimensions reversed, z[b, d-1-i] -- the input of the next block;
 *   log_jac_in       nullable [B,d]: running sum over the previous blocks; log_jac = log_jac_in + this block's
 *                    (same index order as the reference's elementwise `+=`; may alias log_jac). */
int umnn_flow_stack_block_forward(const umnn_mlp* net, const float* x, const float* h, const float* scaling,
                                  const float* cc_w, const float* cc_s, int nb_steps,
                                  long long B, int d, int E, int reverse_z, const float* log_jac_in,
                                  float* z, float* log_jac, float* f_x, float* f_x0, void* stream);

/* umnn_cc_forward / umnn_flow_stack_block_forward / umnn_cc_backward with bf16 or fp32 activation storage (see umnn_io). */
int umnn_cc_forward_io(const umnn_mlp* net, const umnn_io* io, const void* x0, const void* x, const void* h,
                       const float* cc_w, const float* cc_s, int nb_steps,
                       long long B, int d, int E, int inv_f, void* F, void* f_x, void* f_x0, void* stream);
int umnn_flow_stack_block_forward_io(const umnn_mlp* net, const umnn_io* io, const void* x, const void* h,
                                     const float* scaling, const float* cc_w, const float* cc_s, int nb_steps,
                                     long long B, int d, int E, int reverse_z, const void* log_jac_in,
                                     void* z, void* log_jac, void* f_x, void* f_x0, void* stream);
/* umnn_cc_backward_io also takes inv_f (io may be null = fp32 storage): the backward of an integral of 1/f,
 * ParallelNeuralIntegral.apply(..., inv_f=True) -- d_theta and d_h differentiate 1/f (computeIntegrand, ParallelNeuralIntegral.py:70-72),
 * d_x / d_x0 keep f(x) g and -f(x0) g exactly as the reference's backward returns them (:117-123). */
int umnn_cc_backward_io(const umnn_mlp* net, const umnn_io* io, const void* x0, const void* x, const void* h,
                        const void* g, const void* g_fx,
                        const float* cc_w, const float* cc_s, int nb_steps, long long B, int d, int E, int inv_f,
                        void* dx0, void* dx, void* dh, float* dtheta,
                        void* workspace, long long workspace_bytes, void* stream);

/* One link of UMNNMAFFlow.compute_ll (UMNNMAFFlow.py:109-119) with the WHOLE log-likelihood arithmetic inside the
 * launch: besides z (reversed for the next block when reverse_z != 0) the kernel keeps the per-sample running sum
 *   ll[b]  = (first ? 0 : ll[b]) + sum_i log_jac[b,i]            (UMNNMAF.compute_log_jac, UMNNMAF.py:136-139)
 *   ll[b] += -1/2 * sum_i (log(2 pi) + z[b,i]^2)   when last != 0  (UMNNMAFFlow.py:116-118)
 * so a flow's compute_ll is exactly nb_flow x (conditioner + this launch): no [B,d] log_jac accumulation between
 * blocks, no elementwise epilogue kernels.  The row sum is taken by the last tile to deliver a piece of the row
 * (arrival counters + device-scope fences), in a fixed order: bit-reproducible, no floating-point atomics.
 *   log_jac_scratch  [B,d] write-then-read scratch of this launch (this block's log_jac; may be reused by the next)
 *   row_counters     [B] uint32, ZERO on entry; the kernel leaves them zero again
 *   z must not alias x. */
int umnn_flow_ll_block_forward(const umnn_mlp* net, const float* x, const float* h, const float* scaling,
                               const float* cc_w, const float* cc_s, int nb_steps,
                               long long B, int d, int E, int reverse_z, int first, int last,
                               float* z, float* log_jac_scratch, float* ll, unsigned* row_counters, void* stream);

/* Sampling direction, one flow dimension per call: replaces the inner loops of UMNNMAF.invert (UMNNMAF.py:195-231) for
 * dimension j -- `iters` rounds of the 10-candidate bracket search on [-50, 50], each candidate's image being
 * exp(scaling_j) * (h[b, 0*d+j] + int_0^cand f(t; h[b, :, j]) dt) -- for all B samples in ONE launch.
 *   h      [B, E*d]  conditioner output for the current x_inv (dimensions < j already final; MADE is autoregressive,
 *                    so the caller runs it once per dimension, exactly like the reference :198)
 *   z      [B, d]    targets (column j is read);   x_inv [B, d]: column j is WRITTEN (the last round's best candidate)
 * The bracket after k rounds is one candidate step wide, [cand_m, cand_m+1] or [cand_m-1, cand_m]: the returned candidate lies within
 * 100 / 9^iters of the solution, up to what the forward error of the images can move a decision by.  A target beyond G(-50) / G(50)
 * ends on that end exactly -- while the ten fp32 distances |G - z| still differ: for a target so large that they all round to the same
 * value (+-inf included) the tie goes to candidate 0, as in the reference's argmin, and the search ends near -50 (umnn_cc_solve handles
 * such targets).  A sample whose target z[b, j] or whose embedding h[b, :, j] holds a NaN returns NaN in x_inv[b, j] (in
 * every arithmetic mode, after the queued bf16 pass of the fp16-piece mode as well); every other sample is unaffected.
 * UMNN_EUNSUPPORTED for nets with a single hidden layer or images beyond 160 KiB of LDS (callers keep their own loop). */
int umnn_flow_invert_dim(const umnn_mlp* net, const float* h, const float* z, const float* scaling,
                         const float* cc_w, const float* cc_s, int nb_steps,
                         long long B, int d, int E, int j, int iters, float* x_inv, void* stream);

/* Inverse of the monotone map, one dimension per call, for all B rows in ONE launch: solves
 *     scale_b * (off_b + int_0^{x_b} f(t; h[b, :, j]) dt) = target_b        for x_b in [lo, hi]
 * by a safeguarded Newton iteration.  Every quadrature also yields f(x) = dF/dx (node 0 is x), so an iteration is one integral:
 * the residual r tightens the bracket by its sign, the next iterate is x - r / (scale f(x)), replaced -- when it leaves the
 * bracket or is not finite -- by the endpoint it overshot (each endpoint once) or by the bracket's midpoint.  A row stops when
 * |r| <= tol * max(1, |target|), when its bracket has collapsed to adjacent floats or x has stopped changing; a target beyond
 * G(lo) / G(hi) -- an infinite one included -- ends on that endpoint with UMNN_SOLVE_CLAMPED.  The launch ends when every row has stopped or after max_iter
 * iterations (rows still running then carry UMNN_SOLVE_CAPPED and their last evaluated x).
 *   h        [B, E*d]  embedding in the flow's stride-d layout; d = 1, j = 0 is the plain h [B, E] of MonotonicNN
 *   target   column j of rows of t_stride floats (a [B, d] z: t_stride = d; a [B] vector: t_stride = 1, j = 0 with d = 1)
 *   scale    scale_row [B] when non-null, else exp(scaling[j]) when scaling [d] is non-null, else 1
 *   off      off_row [B] when non-null, else h[b, 0*d + j] (embedding row 0, the flow's offset) when off_h0 != 0, else 0
 *   x        column j of rows of x_stride floats is WRITTEN (x_inv[:, j] of a [B, d] tensor in place); must not alias h / target
 *   f_x      nullable [B]: f(x_b; h_b) at the returned x       status  nullable [B]: evaluations used | UMNN_SOLVE_* flags
 * Arithmetic modes, the fp16-piece overflow protocol (an overflowing row is redone by the queued BF16X3 build; in the other modes
 * it returns NaN with UMNN_SOLVE_NONFINITE) and net coverage are those of umnn_flow_invert_dim; UMNN_EUNSUPPORTED otherwise. */
#define UMNN_SOLVE_EVALS_MASK 0xffff
#define UMNN_SOLVE_CLAMPED (1 << 16)
#define UMNN_SOLVE_CAPPED (1 << 17)
#define UMNN_SOLVE_NONFINITE (1 << 18)
int umnn_cc_solve(const umnn_mlp* net, const float* h, const float* target, long long t_stride,
                  const float* scale_row, const float* scaling, const float* off_row, int off_h0,
                  const float* cc_w, const float* cc_s, int nb_steps, long long B, int d, int E, int j,
                  float lo, float hi, float tol, int max_iter,
                  float* x, long long x_stride, float* f_x, int* status, void* stream);

/* umnn_cc_solve that also accumulates the log-Jacobian of the map at the x it returns -- the density of a sample from the solves that
 * drew it (UMNNMAFFlow.sample_and_log_prob).  The last quadrature of a row's solve has x as its node 0, so f(x) is in registers:
 *     lj_row[b] = (lj_first ? 0 : lj_row[b]) + log(f(x_b) + 1e-10) + s,
 *     s = scaling[j] when scaling is non-null (the stored value), else log(scale_row[b]) when scale_row is, else 0
 * written by the wave that publishes row b: one writer per row and launch, a plain read-modify-write, bit-reproducible.  Calling it
 * for j = 0..d-1 with lj_first = 1 on the first call leaves sum_j log|dG_j/dx_j| in lj_row; lj_first = 1 overwrites whatever the
 * buffer held.  lj_row [B] nullable (then exactly umnn_cc_solve); must not alias the other operands.  A row that ends
 * UMNN_SOLVE_NONFINITE makes lj_row[b] NaN; UMNN_SOLVE_CLAMPED / _CAPPED rows add the value at the x they return.  Under the
 * fp16-piece overflow protocol a row the first launch defers adds nothing there and is added by the queued pass: every row is
 * counted once in every arithmetic mode.  Same kernels, launch plan and launch count as umnn_cc_solve. */
int umnn_cc_solve_lj(const umnn_mlp* net, const float* h, const float* target, long long t_stride,
                     const float* scale_row, const float* scaling, const float* off_row, int off_h0,
                     const float* cc_w, const float* cc_s, int nb_steps, long long B, int d, int E, int j,
                     float lo, float hi, float tol, int max_iter,
                     float* x, long long x_stride, float* f_x, int* status, float* lj_row, int lj_first, void* stream);

/* The same solve for every (row, dimension) pair of a flow block in ONE launch -- the inverse of a block under a GIVEN embedding, the
 * step of the Jacobi iteration behind invert(method="jacobi"): for every (b, i)
 *     scale_i * (off_bi + int_0^{x_bi} f(t; h[b, :, i]) dt) = target[b, i]        for x_bi in [lo, hi],
 * scale_i = exp(scaling[i]) (1 when scaling is null), off_bi = h[b, 0*d + i] when off_h0 != 0, else 0.  The iteration, the stop rules,
 * the status word, the arithmetic modes with the fp16-piece overflow protocol, the net coverage (UMNN_EUNSUPPORTED otherwise) and the
 * launch count (an fp16-piece launch and its queued pass count as one) are those of umnn_cc_solve.
 *   h        [B, E*d]  embedding in the flow's stride-d layout        target, x, f_x (nullable), status (nullable)   [B, d]
 *   rows     the forward kernels' mapping: lane p of tile k holds the flat index q = 16 k + p over B*d, b = q / d, i = q - b d (a tile
 *            straddles samples and dimensions; scale and offset are per lane).  Both launch plans apply with ceil(B d / 16) tiles.
 *   x_init   nullable [B, d]: a row's first iterate is x_init[b, i] clamped into [lo, hi] instead of 0 clamped; a non-finite entry means
 *            a cold start (0) for that row.  May alias x.  When it does, a row the fp16-piece launch defers to the queued bf16 pass has
 *            lost its start value to the NaN marker and restarts cold there (same solution, more evaluations). */
int umnn_cc_solve_block(const umnn_mlp* net, const float* h, const float* target, const float* scaling, int off_h0,
                        const float* x_init, const float* cc_w, const float* cc_s, int nb_steps,
                        long long B, int d, int E, float lo, float hi, float tol, int max_iter,
                        float* x, float* f_x, int* status, void* stream);

/* Replaces integrate(..., compute_grad=True) + the Leibniz terms -- ParallelNeuralIntegral.py:66-94,
 * 110-123 (NeuralIntegral.py:47-58,69-75,90-99).  g is grad_output [B,d] (cotangent of F).
 *   g_fx    nullable [B,d]: cotangent of the f_x output of umnn_cc_forward.  The reference gets this
 *           term from ordinary autograd through `self.net.forward(x)` (UMNNMAF.py:138,143,148); here it
 *           is one more VJP at quadrature node 0, including d f/d x.
 *   dtheta  [n_params] in integrand.parameters() order (W0,b0,W1,b1,...); OVERWRITTEN
 *   dh      [B,E*d]; dx, dx0 [B,d]  (dx = f(x;h)*g [+ g_fx * df/dx], dx0 = -f(x0;h)*g); each nullable.
 *   workspace: device scratch of at least umnn_cc_backward_workspace_bytes() bytes (which never shrinks as B grows: a workspace
 *   sized for the largest batch serves every smaller one). */
int umnn_cc_backward(const umnn_mlp* net, const float* x0, const float* x, const float* h,
                     const float* g, const float* g_fx,
                     const float* cc_w, const float* cc_s, int nb_steps,
                     long long B, int d, int E,
                     float* dx0, float* dx, float* dh, float* dtheta,
                     void* workspace, long long workspace_bytes, void* stream);
long long umnn_cc_backward_workspace_bytes(const umnn_mlp* net, long long B, int d, int E);

/* Multi-output quadrature (cc_multi.hip): K = net->widths[n_linear] in [2, UMNN_MAX_OUTPUTS] integrands f_k(t; h) that share every
 * hidden layer -- the last Linear is W_L [K, H_L], b_L [K], the output activation is applied per component -- integrated in ONE
 * launch: F[b,i,k] = int_{x0}^{x} f_k(t; h[b,:,i]) dt.  F, f_x, f_x0 and g are [B, d, K], k minor.  Exact fp32 MFMA and fp32
 * storage whatever umnn_set_forward_precision / umnn_set_backward_precision say.  x0, f_x, f_x0 and every gradient output may
 * be NULL as in the single-output entries; B == 0 returns 0.  The backward has the reference's convention summed over k:
 *   dx[b,i] = sum_k g_k f_k(x), dx0[b,i] = -sum_k g_k f_k(x0)   (f itself under inv_f too, like umnn_cc_backward_io);
 *   dtheta  flat in parameters() order, W_L as [K, H_L] and b_L as [K]; OVERWRITTEN;  dh [B, E*d].
 * umnn_cc_backward_multi_fx also takes g_fx [B, d, K] (k minor; may be NULL), the cotangent of f_x[b,i,k] = f_k(x; h) -- f itself,
 * also under inv_f, like umnn_cc_backward_io's: the output layer's cotangent at node x gains g_fx,k out'(s_k), which reaches dh and
 * dtheta through the same sweep, and
 *   dx[b,i] = sum_k g_k f_k(x) + sum_k g_fx,k df_k/dx (x).
 * Same workspace (umnn_cc_backward_multi_workspace_bytes), argument checks and launch notes; umnn_cc_backward_multi is that call
 * with g_fx = NULL and runs the kernels it always ran (a g_fx selects builds of the same passes that carry it).  No float
 * atomics: two runs are bit-identical.  UMNN_EUNSUPPORTED when the weight images of the net exceed the LDS.  Every other entry
 * point keeps rejecting widths[n_linear] != 1. */
int umnn_cc_forward_multi(const umnn_mlp* net, const float* x0, const float* x, const float* h,
                          const float* cc_w, const float* cc_s, int nb_steps, long long B, int d, int E, int inv_f,
                          float* F, float* f_x, float* f_x0, void* stream);
int umnn_cc_backward_multi(const umnn_mlp* net, const float* x0, const float* x, const float* h, const float* g,
                           const float* cc_w, const float* cc_s, int nb_steps, long long B, int d, int E, int inv_f,
                           float* dx0, float* dx, float* dh, float* dtheta,
                           void* workspace, long long workspace_bytes, void* stream);
int umnn_cc_backward_multi_fx(const umnn_mlp* net, const float* x0, const float* x, const float* h, const float* g, const float* g_fx,
                              const float* cc_w, const float* cc_s, int nb_steps, long long B, int d, int E, int inv_f,
                              float* dx0, float* dx, float* dh, float* dtheta, void* workspace, long long workspace_bytes, void* stream);
long long umnn_cc_backward_multi_workspace_bytes(const umnn_mlp* net, long long B, int d, int E);

/* Whole curves from one quadrature (cc_multi.hip, cc_cumulate.hip; d = 1, fp32 storage, exact fp32 MFMA).
 * umnn_cc_forward_multi_nodes: umnn_cc_forward_multi (same plan, grid and arithmetic; no inv_f, f_x, f_x0) that also stores the
 * integrand at every node, f_nodes[b][j][k] = f_k(t_j; h_b), [B, nb_steps + 1, K], k minor; node j = 0 is x, j = nb_steps is x0.
 * K = net->widths[n_linear] in [1, UMNN_MAX_OUTPUTS] here (a single output too); d must be 1; F [B,K] and f_nodes non-null.
 * umnn_cc_cumulate: out[q][n - i][k] = (x_q - x0_q)/2 * sum_j Q[i][j] values[q][j][k] for n = nb_steps, i, j = 0..n: with Q the
 * fp32 [n+1, n+1] table of umnn_amd.quadrature.cc_cumulative_matrix (row i: the integral of the quadrature's interpolant from x0
 * to node i) and values the f_nodes above, out[q][i'][k] is the integral from x0 to the i'-th abscissa counted FROM THE LOWER
 * LIMIT: out[q][0] = 0 exactly, out[q][n] the F of the forward up to rounding.  values, out [NI, n+1, K], k minor, 1 <= K <=
 * UMNN_MAX_OUTPUTS; x0 may be NULL (zeros).  The kernel applies whatever table it is given (the same table with its columns
 * reversed takes values stored in ascending order).  No atomics: two runs are bit-identical.  UMNN_EUNSUPPORTED for nb_steps >
 * 127 (the table's LDS image is budgeted at 64 KiB); NI == 0 returns 0.  Both note their kernel through the launch notes. */
int umnn_cc_forward_multi_nodes(const umnn_mlp* net, const float* x0, const float* x, const float* h,
                                const float* cc_w, const float* cc_s, int nb_steps, long long B, int d, int E,
                                float* F, float* f_nodes, void* stream);
int umnn_cc_cumulate(const float* Q, const float* values, const float* x0, const float* x, int nb_steps, long long NI, int K,
                     float* out, void* stream);

/* The backward of a curve (cc_multi.hip, cc_cumulate.hip; d = 1, fp32 storage, exact fp32 MFMA, no float atomics: two runs are
 * bit-identical).
 * umnn_cc_backward_multi_nodes: the multi-output backward with a cotangent PER NODE, cot_nodes[b][j][k] of f_k(t_j; h_b), [B,
 * nb_steps + 1, K], k minor, in the node order of f_nodes above (node 0 is x).  K in [1, UMNN_MAX_OUTPUTS], d must be 1.
 *   dh, dtheta = sum_j VJP_f(t_j, h)[cot_nodes[:, j]]                     (dtheta OVERWRITTEN, flat in parameters() order)
 *   dx  = sum_j (u_j / 2)     tau_j,    dx0 = sum_j (1 - u_j / 2) tau_j,   tau_j = sum_k cot_nodes[b][j][k] df_k/dt (t_j),
 * u_j = cc_s[j] + 1: what the limits do through the nodes t_j = x0 + (x - x0) u_j / 2.  There is no quadrature weight, no span
 * factor and no Leibniz term in it -- the caller owns them -- and no division by x - x0: a row with x == x0 is an ordinary row.
 * The passes, the finishing kernels and the workspace layout are umnn_cc_backward_multi_fx's (the node-cotangent builds of the same
 * passes); the workspace size is umnn_cc_backward_multi_nodes_workspace_bytes -- umnn_cc_backward_multi_workspace_bytes's figure,
 * answered for K = 1 too.  UMNN_EUNSUPPORTED as umnn_cc_backward_multi_fx; B == 0 launches nothing and zeroes dtheta.
 * umnn_cc_cumulate_adjoint: out[q][j][k] = sum_i Qt[j][i] g[q][i][k], i, j = 0..nb_steps: umnn_cc_cumulate's product alone, with
 * no span factor and no reversed output index.  With Qt the transpose of the table umnn_cc_cumulate applied -- its rows reversed,
 * so that g is indexed from the lower limit like that entry's output (umnn_amd.quadrature.device_cumulative_adjoint) -- out is the
 * cotangent of its `values` up to the factor (x - x0)/2.  Same limits and answers as umnn_cc_cumulate. */
int umnn_cc_backward_multi_nodes(const umnn_mlp* net, const float* x0, const float* x, const float* h, const float* cot_nodes,
                                 const float* cc_s, int nb_steps, long long B, int d, int E,
                                 float* dx0, float* dx, float* dh, float* dtheta,
                                 void* workspace, long long workspace_bytes, void* stream);
long long umnn_cc_backward_multi_nodes_workspace_bytes(const umnn_mlp* net, long long B, int E);
int umnn_cc_cumulate_adjoint(const float* Qt, const float* g, int nb_steps, long long NI, int K, float* out, void* stream);

/* Inverse of a weighted sum of the K monotone outputs, for all B rows in ONE launch (cc_multi.hip; MonotonicNN's shape, d = 1): solves
 *     sum_k coef[b,k] * int_0^{x_b} f_k(t; h_b) dt = target[b]        for x_b in [lo, hi]
 * with coef >= 0 and a positive entry per row (not checked) -- the event time of K competing risks, a quantile of a mixture of K
 * CDFs.  The iteration is umnn_cc_solve's, word for word, on S = sum_k coef_k F_k(x) and D = sum_k coef_k f_k(x): start at 0 clamped
 * into [lo, hi]; the residual r = S - target tightens the bracket by its sign; the next point is x - r / D, or the endpoint it
 * overshot (each endpoint once, while not yet evaluated), or the bracket's midpoint; a row stops when |r| <= tol * max(1, |target|),
 * when x sits on the endpoint the target lies beyond (UMNN_SOLVE_CLAMPED; a row of zero coefficients ends so), when its bracket has
 * collapsed or x has stopped changing; rows still running after max_iter evaluations carry UMNN_SOLVE_CAPPED and their last
 * evaluated x.  One iteration is one K-output quadrature (the node loop of umnn_cc_forward_multi with upper limit x): exact fp32
 * MFMA whatever the precision options say, no atomics, two runs are bit-identical.
 *   h [B,E]   target [B]   coef [B,K], k minor, K = net->widths[n_linear] in [2, UMNN_MAX_OUTPUTS] (anything else: UMNN_EINVAL)
 *   x [B]     F, f_x [B,K] nullable: F_k and f_k at the returned x     status [B] nullable: the word of umnn_cc_solve
 * A row whose target, embedding or coefficients hold a NaN returns NaN in x with UMNN_SOLVE_NONFINITE; every other row is
 * unaffected.  A non-finite F_k marks its row UMNN_SOLVE_NONFINITE under a zero coefficient as well (0 * inf is a NaN).
 * nb_steps >= 1, 1 <= max_iter <= 65535, lo < hi, tol >= 0, non-null h, target, coef, cc_w, cc_s, x; B == 0 returns 0 and launches
 * nothing.  UMNN_EUNSUPPORTED when the weight images of the net exceed the LDS (callers iterate umnn_cc_forward_multi themselves). */
int umnn_cc_solve_multi(const umnn_mlp* net, const float* h, const float* target, const float* coef,
                        const float* cc_w, const float* cc_s, int nb_steps, long long B, int E,
                        float lo, float hi, float tol, int max_iter,
                        float* x, float* F, float* f_x, int* status, void* stream);

/* Training forward / backward pair for nets of the three-stage backward family (first hidden layer of 5..8 sixteen-feature tiles
 * over 2..4 narrower ones: MNISTExperiment's 31-100-50-50-50-50-1, /root/reference MNISTExperiment.py:238).  That backward recomputes
 * the pre-activations z_2 of hidden layer 2 at every node in its stage A and hands them to stage B through HBM; the forward has just
 * computed the same numbers.  umnn_flow_stack_block_forward_save = umnn_flow_stack_block_forward that also leaves them in z2_save
 * ([tile][node][register][lane] fp32, umnn_cc_forward_z2_floats() floats: 0.83 GB for 100 x 784 integrals at n = 50);
 * umnn_cc_backward_saved = umnn_cc_backward (lower limit 0) that reads them and runs stage A for the tangent element of the g_fx term
 * only.  umnn_cc_forward_z2_floats returns 0 when the pair does not apply (other nets; fwd_precision fp32 / bf16x6; bwd_precision fp32):
 * callers then use the plain entry points.  Trade: memory held from forward to backward for ~0.26 ms per MNIST-shaped block. */
long long umnn_cc_forward_z2_floats(const umnn_mlp* net, long long B, int d, int E, int nb_steps);
int umnn_flow_stack_block_forward_save(const umnn_mlp* net, const float* x, const float* h, const float* scaling,
                                       const float* cc_w, const float* cc_s, int nb_steps,
                                       long long B, int d, int E, int reverse_z, const float* log_jac_in,
                                       float* z, float* log_jac, float* f_x, float* f_x0,
                                       float* z2_save, long long z2_floats, void* stream);
int umnn_cc_backward_saved(const umnn_mlp* net, const float* x, const float* h, const float* g, const float* g_fx,
                           const float* cc_w, const float* cc_s, int nb_steps, long long B, int d, int E,
                           float* dx, float* dh, float* dtheta, const float* z2_saved, long long z2_floats,
                           void* workspace, long long workspace_bytes, void* stream);
/* The pair with bf16 or fp32 activation storage (umnn_io; io may be null = fp32): configuration C4's bf16 embedding on the training path. */
int umnn_flow_stack_block_forward_save_io(const umnn_mlp* net, const umnn_io* io, const void* x, const void* h, const float* scaling,
                                          const float* cc_w, const float* cc_s, int nb_steps,
                                          long long B, int d, int E, int reverse_z, const void* log_jac_in,
                                          void* z, void* log_jac, void* f_x, void* f_x0,
                                          float* z2_save, long long z2_floats, void* stream);
int umnn_cc_backward_saved_io(const umnn_mlp* net, const umnn_io* io, const void* x, const void* h, const void* g, const void* g_fx,
                              const float* cc_w, const float* cc_s, int nb_steps, long long B, int d, int E,
                              void* dx, void* dh, float* dtheta, const float* z2_saved, long long z2_floats,
                              void* workspace, long long workspace_bytes, void* stream);
/* The quadrature backward of one flow block: umnn_cc_backward_saved_io -- or, with z2_saved null, umnn_cc_backward_io with lower limit 0 --
 * whose d_h also carries the block's h_0 term: z = exp(s) (F + h_0) sends the cotangent of F to embedding row 0 as well, and h0_cot
 * ([B, d] fp32, nullable = none) is added to d_h[b, 0 * d + i] in fp32 by the kernel that stores d_h.  A bf16 d_h is thereby rounded
 * once; added afterwards, row 0 would be rounded twice. */
int umnn_cc_backward_block_io(const umnn_mlp* net, const umnn_io* io, const void* x, const void* h, const void* g, const void* g_fx,
                              const float* cc_w, const float* cc_s, int nb_steps, long long B, int d, int E, const float* h0_cot,
                              void* dx, void* dh, float* dtheta, const float* z2_saved, long long z2_floats,
                              void* workspace, long long workspace_bytes, void* stream);

/* Elementwise glue of a block's TRAINING path (umnn_amd/csrc/cc_flow_glue.hip), one launch each.
 * umnn_flow_block_cotangents: backward of the block epilogue (UMNNMAF.py:80-83,134,138-139)
 *     z[b, rev(i)] = exp(s_i) (F[b,i] + h_0[b,i]),  log_jac[b,i] = log(f_x[b,i] + 1e-10) + s_i      (rev(i) = d-1-i if reverse_z)
 *   from the cotangents g_z, g_log_jac [B,d] (either nullable = zero) to gF = exp(s_i) g_z[b, rev(i)] (also the cotangent of h_0) and
 *   g_fx = g_log_jac / (f_x + 1e-10) (g_fx nullable: not wanted) -- the g / g_fx inputs of umnn_cc_backward.
 * umnn_flow_ll_forward / _backward: UMNNMAFFlow.compute_ll's reduction (UMNNMAFFlow.py:109-119)
 *     ll[b] = sum_i log_jac[b,i] - 1/2 sum_i (log 2 pi + z[b,i]^2);   g_log_jac[b,i] = g_ll[b],  g_z[b,i] = -z[b,i] g_ll[b]. */
int umnn_flow_block_cotangents(const float* g_z, const float* g_log_jac, const float* f_x, const float* scaling,
                               long long B, int d, int reverse_z, float* gF, float* g_fx, void* stream);
int umnn_flow_ll_forward(const float* z, const float* log_jac, long long B, int d, float* ll, void* stream);
int umnn_flow_ll_backward(const float* z, const float* g_ll, long long B, int d, float* g_z, float* g_log_jac, void* stream);
/* Log-density of a drawn sample (UMNNMAFFlow.sample_and_log_prob), one launch each, one wave per row, fixed summation order.
 * umnn_flow_sample_lj_rows: lj_row[b] = (first ? 0 : lj_row[b]) + sum_i (log(f_x[b,i] + 1e-10) + scaling[i]) -- a block's log|det J|
 *   from the f_x [B,d] its last Jacobi sweep (umnn_cc_solve_block) wrote; first is 0 or 1.
 * umnn_flow_sample_ll: ll[b] = lj_row[b] - 1/2 sum_i (log 2 pi + z[b,i]^2), z [B,d] the noise the sample was drawn from; ll must not
 *   alias lj_row.  B = 0: no launch. */
int umnn_flow_sample_lj_rows(const float* f_x, const float* scaling, long long B, int d, int first, float* lj_row, void* stream);
int umnn_flow_sample_ll(const float* z, const float* lj_row, long long B, int d, float* ll, void* stream);
/* One adjoint Jacobi sweep's elementwise step (the gradient through a sample x = T^-1(z), umnn_amd/inverse.py): with J = dT/dx lower
 * triangular and D = exp(log_jac) its diagonal, J^T lam = g is iterated as lam <- lam + (g - r) / D, r = J^T lam the block's VJP.
 *     lam_out[q] = lam[q] + (g[q] - r[q]) exp(-log_jac[q])      over the B d entries, all [B,d] fp32; lam_out may be lam.
 * flags[0] (zeroed by the caller) gets bit 0 ORed in when some entry has |g - r| > tol max(1, |g|) and bit 1 when some g - r is not
 * finite; a non-finite entry never sets bit 0.  tol >= 0.  B = 0: no launch. */
int umnn_flow_adjoint_update(const float* g, const float* r, const float* log_jac, const float* lam, long long B, int d, float tol,
                             float* lam_out, unsigned* flags, void* stream);

/* Replaces compute_cc_weights -- ParallelNeuralIntegral.py:14-34: writes nb_steps+1 fp32
 * weights and nodes into HOST buffers (float64 arithmetic, cast at the end). */
int umnn_cc_tables_host(int nb_steps, float* w_host, float* s_host);

/* Algorithmic FLOPs of one forward integral, SURVEY 8(d):
 *   2*[(n+1)*(H1 + sum H_l*H_{l+1} + H_L) + E*H1]. */
double umnn_cc_forward_flops_per_integral(const umnn_mlp* net, int nb_steps);

/* Introspection used by tests, the smoke test and the bench. */
const char* umnn_last_error(void);
int umnn_version(void);
long long umnn_launch_count(void);          /* quadrature kernels (forward / backward / finishing) launched by this process so far */
long long umnn_made_launch_count(void);     /* launches of the conditioner kernels (umnn_made_mlp_forward, umnn_made_linear_forward, umnn_made_step) so far */
const char* umnn_last_made_kernel_name(void);
const char* umnn_last_kernel_name(void);    /* variant picked by the last forward/backward */
/* Times `reps` back-to-back umnn_cc_forward launches with hipEvents recorded on `stream`
 * (the stream the kernels run on) and returns the average milliseconds per launch in *ms. */
int umnn_cc_forward_timed(const umnn_mlp* net, const float* x0, const float* x, const float* h,
                          const float* cc_w, const float* cc_s, int nb_steps,
                          long long B, int d, int E, float* F, float* f_x, float* f_x0,
                          int reps, float* ms, void* stream);

/* Arithmetic of the hidden-layer GEMMs in the FORWARD kernels -- umnn_cc_forward, the umnn_flow_*_forward entry points, their _io
 * forms and umnn_flow_invert_dim (process-wide; default UMNN_PRECISION_F16X3, or the environment variable UMNN_FWD_PRECISION =
 * fp32 | bf16x3 | bf16x6 | f16x3 at first use).  Every mode meets the 1e-4 tolerance of the path with margin (measured max
 * relative error of F on the golden set: fp32 ~4e-7, bf16x6 ~4e-7, f16x3 ~5e-7, bf16x3 ~6e-6; layer 1, the hoisted first-layer
 * term, the output dot product, ELU and the quadrature sum are fp32 in every mode).
 *   F16X3   (default since round 5)  operands split in two fp16 pieces (11 bits each), 3 cross terms on v_mfma_f32_16x16x32_f16,
 *           fp32 accumulation: fp32-level accuracy at the cost of BF16X3.  fp16's exponent range is handled by an overflow
 *           protocol (umnn_amd/csrc/cc_fwd_launch.h): a tile group (16 or 32 integrals) whose quadrature sum is not finite --
 *           where an overflowed piece always ends -- writes only a NaN marker into its slots of F (z for the flow entry points,
 *           x_inv[:, j] for umnn_flow_invert_dim), and the BF16X3 build of the same kernel, queued behind every launch on the
 *           same stream, recomputes exactly the marked groups (one scalar load per workgroup when nothing overflowed).  Those
 *           integrals therefore come back at BF16X3 accuracy -- never NaN unless an input was, never a wrong finite value.  A
 *           launch whose marker output aliases x, x0 or h runs BF16X3 outright.  umnn_launch_count() counts the pair as one.
 *   FP32    v_mfma_f32_16x16x4_f32: exact fp32 products (an fmaf chain), fp32-vector-rate matrix path -- the reference's arithmetic
 *   BF16X3  operands split in two bf16 pieces, 3 cross terms on v_mfma_f32_16x16x32_bf16, fp32 accumulation (the default until round 4)
 *   BF16X6  three bf16 pieces, 6 cross terms: fp32-level accuracy at twice the matrix work
 * umnn_flow_invert_dim: F16X3 and BF16X3 run the in-kernel bracket search for every net the forward covers; FP32 / BF16X6 run it on
 * three bf16 pieces for nets of at most four 16-feature tiles per layer and on two fp16 pieces (the F16X3 search: fp32-level
 * products, overflowing samples redone on bf16 pieces) for wider ones, whose three-piece form does not fit the register file. */
#define UMNN_PRECISION_FP32 0
#define UMNN_PRECISION_BF16X3 1
#define UMNN_PRECISION_BF16X6 2
#define UMNN_PRECISION_F16X3 3
int umnn_set_forward_precision(int mode);
int umnn_get_forward_precision(void);
/* Arithmetic of the BACKWARD kernels (umnn_cc_backward, _io): UMNN_PRECISION_BF16X3 (default) or UMNN_PRECISION_FP32 (env
 * UMNN_BWD_PRECISION = bf16x3 | fp32).  Under both, d_x0 / d_x Leibniz terms, the output layer, dc and every reduction are fp32.
 *   BF16X3  the matrix-core kernels.  The forward recompute inside them is always fp32-LEVEL (the sign of every hidden
 *           pre-activation decides a LeakyReLU slope): six cross terms on three bf16 pieces, or three cross terms on two fp16
 *           pieces; the delta chain and the dW products carry three cross terms.  Which kernel runs:
 *           (the exact rules -- sizes, thresholds, eligibility -- are csrc/cc_bwd_plan.h: bwd_route; umnn_cc_backward_plan_name asks it)
 *             - four hidden layers of 32..63 units at batches that fill the workgroups:
 *               the eight-wave workgroup pipeline -- on fp16 pieces (cc_bwd_ws16_kernel.h, kernel names cc_bwd_f16<...,WS>) for
 *               large launches (option bwd_ws16 = 1; 2 = whenever eligible; 0 = never), on bf16 pieces
 *               (cc_bwd_ws_kernel.h, cc_bwd_bf16<...,WS>) otherwise and for 1/f launches and sigmoid outputs.  The fp16 kernel
 *               carries cotangents scaled by a per-launch power of two (cc_bwd_cotmax_kernel), detects an overflowed piece in
 *               its output-layer and dc sums, raises a flag word in the workspace, and the bf16 pipeline queued behind it
 *               rewrites every output when -- and only when -- the flag is set.  Measured against a float64 run of the reference
 *               algorithm at the benchmarked size (8192 x 63 x 101 nodes): d_theta 5.8e-5 of its largest entry (exact-fp32
 *               kernels 3.1e-5, a float32 ATen run of the reference's own algorithm 2.7e-5, the bf16 pipeline 2.4e-4);
 *             - two or three hidden layers of 32..63 units, or small batches: the software-pipelined one-pass loop
 *               (cc_bwd_swp_kernel.h; option bwd_swp = 0: the round-2 loop);
 *             - a first hidden layer of 5..8 tiles over 2..4 narrower ones (31-100-50-50-50-50-1): three stages through HBM
 *               (cc_backward_front.hip) -- stages A and B on fp16 pieces for single-chunk calls under the same rule, with
 *               their bf16 builds queued as the overflow fallback, on bf16 pieces otherwise;
 *             - every other shape: the fp32 kernels below.
 *   FP32    exact fp32 MFMA (cc_backward.hip) for every one-pass shape; the three-stage family runs its build with three bf16
 *           pieces / six cross terms in EVERY product (cc_backward_front_p3.hip, kernel names cc_bwd_bf16x6<...>): fp32-level,
 *           not fp32 instructions.
 * Narrower layers of a 32..63-wide net are zero-padded to four 16-feature tiles by the staged weight images. */
/* Which kernel family umnn_cc_backward would run for this net: 1 shape-exact kernels (one pass; or, for a first hidden layer
 * of 5..8 sixteen-feature tiles over 2..4 narrower ones such as MNISTExperiment's 100-50-50-50-50, the three-stage kernels
 * of cc_backward_front.hip -- under UMNN_PRECISION_FP32 their build with six bf16 cross terms in every product, fp32-level; or, for unequal hidden widths of 64..127, the shape-exact fp32 kernels of
 * the 5- / 7- / 8-tile family that holds the widest layer, the narrower layers zero-padded virtually), 0 generic kernels with
 * at most four tiles per layer, -1 generic kernels with more tiles (deep wide nets whose zero-padded weight images exceed the
 * LDS: they spill registers and are ~100x slower -- the shipped host code sends such nets to the materialised ATen chain on the
 * GPU), < -1 error.  The staged family takes its HBM scratch from the
 * workspace (umnn_cc_backward_workspace_bytes includes up to 2 GiB for it). */
int umnn_cc_backward_kind(const umnn_mlp* net, int E);
/* The name umnn_last_kernel_name_of(UMNN_PROF_BACKWARD) would hold after umnn_cc_backward_io(net, ..., nb_steps, B, d, E, ...) under the
 * current options, "" where that call would return an error.  flags: UMNN_PLAN_* bits for what the call brings.  Read-only: the launch
 * plan (csrc/cc_bwd_plan.h) is evaluated and nothing is launched, so it also answers without a device (as for 256 CUs). */
#define UMNN_PLAN_INV_F 1            /* inv_f != 0 */
#define UMNN_PLAN_G_FX 2             /* g_fx != NULL */
#define UMNN_PLAN_Z2_SAVED 4         /* umnn_cc_backward_saved(_io) with a z_2 buffer */
#define UMNN_PLAN_X_BF16 8           /* umnn_io::x_dtype = UMNN_DTYPE_BF16 */
#define UMNN_PLAN_H_BF16 16          /* umnn_io::h_dtype = UMNN_DTYPE_BF16 */
const char* umnn_cc_backward_plan_name(const umnn_mlp* net, long long B, int d, int E, int nb_steps, int flags);
/* The launch plan of a forward, bracket-search or Newton-solve call of this net and shape under the current options: what
 * umnn_last_kernel_name() would hold afterwards, and the quantities the name does not show (P and ns decide the summation order,
 * hence the bits).  kind: UMNN_PLAN_FORWARD (umnn_cc_forward*, umnn_flow_*_forward*: B x d integrals), UMNN_PLAN_SEARCH
 * (umnn_flow_invert_dim: B samples), UMNN_PLAN_SOLVE (umnn_cc_solve: B rows), UMNN_PLAN_SOLVE_BLOCK (umnn_cc_solve_block: B x d rows).
 * flags (forward only): UMNN_PLAN_Z2_SAVED (umnn_flow_stack_block_forward_save*), UMNN_PLAN_MARKER_ALIASED (F, or z for the flow entry
 * points, aliases x, x0 or h); the storage flags UMNN_PLAN_X_BF16 / UMNN_PLAN_H_BF16 are accepted and do not route.  Returns 0 and
 * fills *out (all zero, name "", for B = 0), or the code -- with the text in umnn_last_error() -- the entry point itself would return
 * for this net and shape, leaving name "".  Read-only: the plan (csrc/cc_fwd_plan.h) is evaluated and nothing is launched, so it also
 * answers without a device (as for 256 CUs). */
#define UMNN_PLAN_FORWARD 0
#define UMNN_PLAN_SEARCH 1
#define UMNN_PLAN_SOLVE 2
#define UMNN_PLAN_SOLVE_BLOCK 3
#define UMNN_PLAN_MARKER_ALIASED 32  /* the marker output of a forward call aliases one of its inputs */
typedef struct umnn_launch_plan_info {
    const char* name;        /* kernel name (static storage) */
    int pieces;              /* 16-bit pieces per operand: 2 or 3; 0 = fp32 MFMA */
    int P, ns;               /* point tiles per wave; node-range split */
    int waves_per_block;
    long long blocks, lds_bytes;
    int fallback;            /* 1: the bf16 build of the same variant is queued behind the launch (fp16 pieces) */
} umnn_launch_plan_info;
int umnn_cc_launch_plan(const umnn_mlp* net, int kind, long long B, int d, int E, int nb_steps, int flags, umnn_launch_plan_info* out);
int umnn_set_backward_precision(int mode);
int umnn_get_backward_precision(void);

/* Launch options.  The UMNN_* environment variables are read once per process -- at first use or on
 * umnn_reload_env() -- and live in atomics afterwards, so the launch path never calls getenv.  Names:
 * "fwd_precision", "bwd_precision" (UMNN_PRECISION_*), "fwd_p" (1|2), "fwd_ns" (1|2|4; a split into more parts than
 * the nb_steps + 1 nodes runs whole, as the automatic rule does), "fwd_tail" (0|1), "fwd_pipe"
 * (0 plain loop | 1 pipelined 16x16x32 loop, default | 2 the 32x32x16 formulation of the 48..51-wide shapes),
 * "fwd_pad", "fwd_pad_min", "bwd_ns" (1..32), "bwd_swp" (1: software-pipelined one-pass bf16 backward, default; 0: the
 * round-2 node loop), "bwd_ws" (1, default: four-hidden-layer nets at large batch take the weight-stationary workgroup
 * pipeline, cc_bwd_ws_kernel.h; 0: they stay on the one-pass loop), "bwd_ws16" (that pipeline on fp16 pieces,
 * cc_bwd_ws16_kernel.h -- three-term recompute, cotangents scaled by a per-launch power of two, overflow flag + queued bf16
 * fallback: 1, default: large launches, the threshold being bwd_ws16_ok of csrc/cc_bwd_plan.h; 2: whenever the pipeline is eligible;
 * 0: never), "front_bwd2" (1,
 * default: the last stage of the three-stage backward runs two waves per tile of integrals, each on half of the wide first hidden
 * layer's feature tiles -- on fp16 pieces behind the fp16 middle stage, its bf16 build queued as the overflow fallback; 2: two waves,
 * bf16 pieces always; 0: one wave per tile);
 * -1 = automatic for the tuning knobs.  "fwd_precision" defaults to UMNN_PRECISION_F16X3 (see above). */
int umnn_set_option(const char* name, int value);
int umnn_get_option(const char* name, int* value);
int umnn_reload_env(void);

/* Per-launch timing: while enabled, every forward/backward launch is bracketed by hipEvents recorded on its own
 * launch stream.  umnn_profile_read synchronises on them and returns the summed kernel milliseconds, the number of
 * launches and the summed algorithmic FLOPs (forward launches only carry FLOPs).  enable(0/1) clears the records. */
int umnn_profile_enable(int on);
int umnn_profile_read(double* total_ms, long long* launches, double* total_flops);
/* The same per class of launch: forward quadrature kernels (FLOPs = the algorithmic forward count), the main backward
 * kernels (FLOPs = 3 x the forward count of the same integrals: 2 x for the two gradient GEMMs per forward GEMM + 1 x for the
 * forward recompute, SURVEY 8d "Backward ~ 2x forward MACs + recompute"), and the finishing kernels of the backward
 * (dc sum, d_h, dW1, d_theta reduction; bracketed as one record, no FLOPs). */
#define UMNN_PROF_FORWARD 0
#define UMNN_PROF_BACKWARD 1
#define UMNN_PROF_FINISH 2
int umnn_profile_read_tag(int tag, double* total_ms, long long* launches, double* total_flops);
/* Variant name of the last launch of that class by ANY thread (umnn_last_kernel_name is per calling thread, and the
 * backward runs on autograd worker threads). */
const char* umnn_last_kernel_name_of(int tag);

/* MADE conditioner operand builder (reference models/UMNN/made.py:16-27: MaskedLinear chains around ReLU).  Reads the
 * previous layer's raw fp32 output x [rows, cols] and writes, per row, the bf16 operand
 *   [ hi(a) | lo(a) | hi(a) | 1 | 1 | 0 ... ]  (ld_out >= 3*cols+2 bf16 per row),  a = relu ? max(x,0) : x,
 * hi/lo = round-to-nearest bf16 pieces of a.  Multiplied (one bf16 GEMM, fp32 accumulate) by the host-packed weights
 * [Wh | Wh | Wl | bh | bl | 0...] it gives W a + b to ~3e-6 of the output range. */
int umnn_made_split3(const float* x, long long rows, int cols, int relu, void* out_bf16, int ld_out, void* stream);

/* The whole MADE conditioner of one flow block as ONE launch (reference models/UMNN/made.py:16-27 MaskedLinear, :113-119
 * MADE.forward, :165-168 ConditionnalMADE.forward; called once per block, UMNNMAF.py:79):
 *     h = W_L relu( ... relu(W_1 x + b_1) ... ) + b_L,   x [B, widths[0]] fp32  ->  h [B, widths[n_layers]] fp32 or bf16.
 * W[l]: the MASKED weight of layer l as bf16 MFMA fragments [tile t][K-step s][piece (hi, lo)][lane 64][8 bf16], lane
 * (g = lane>>4, rho = lane&15) slot j holding piece(W[16 t + rho][32 s + 16 (j>>2) + 4 g + (j&3)]) (zero outside the matrix)
 * -- the K order in which the kernel's accumulators become the next layer's operand; b[l]: fp32 bias.  Input and hidden
 * widths up to 512 (UMNN_EUNSUPPORTED beyond: the caller keeps the library GEMMs); products as xh Wh + xl Wh + xh Wl with
 * fp32 accumulation (the arithmetic of umnn_made_split3's GEMMs), bias added in fp32. */
#define UMNN_MADE_MAX_LAYERS 8
typedef struct umnn_made_net {
    int n_layers;
    int widths[UMNN_MADE_MAX_LAYERS + 1];
    const void* W[UMNN_MADE_MAX_LAYERS];
    const float* b[UMNN_MADE_MAX_LAYERS];
} umnn_made_net;
int umnn_made_mlp_forward(const umnn_made_net* net, const float* x, long long B, void* h_out, int out_bf16, void* stream);
/* The same kernel with the output format spelt out: out_mode 0 fp32 h, 1 bf16 h, 2 = the masked MLP's HIDDEN stack only -- the last
 * layer given here is followed by ReLU and written as umnn_made_split3's operand [hi | lo | hi | 1 | 1 | 0...] (out_ld bf16 per row)
 * for a wide output layer that stays a library GEMM (BSDS300's 1890, the VAE flow's 1920 columns). */
int umnn_made_mlp_forward_ex(const umnn_made_net* net, const float* x, long long B, void* out, int out_mode, int out_ld, void* stream);
/* ONE masked linear layer as its own launch (made.py:16-27 MaskedLinear.forward = F.linear(input, mask * weight, bias)), for
 * conditioners whose OUTPUT layer is wide (the VAE flow's 1920, BSDS300's 1890 columns), where one workgroup per row group cannot
 * fill the chip: the grid is (row groups of 16*row_tiles rows) x (feature_groups groups of output tiles); the bf16 split of the
 * input happens in the operand load (relu_in != 0: the input is the previous layer's pre-activation and ReLU is applied on load, so
 * a hidden layer needs no separate activation / split launch); x2 != NULL: the input is [x | x2] with x [B, K1] and x2 [B, K - K1]
 * (ConditionnalMADE's cat((context, x), 1), made.py:167, without the copy); out = in' W^T + b as fp32 (out_bf16 == 0) or bf16.
 * W_frag / bias / arithmetic as in umnn_made_net; K <= 512.  row_tiles 0 (auto) | 1 | 2 | 4; feature_groups 0 (auto) or a count. */
int umnn_made_linear_forward(const void* W_frag, const float* bias, int K, int N, const float* x, const float* x2, int K1,
                             long long B, int relu_in, void* out, int out_bf16, int row_tiles, int feature_groups, void* stream);

/* Training chain of the conditioner (csrc/made_train.hip; replaces, per masked linear, the ReluBackward / bias-reduction / mask
 * product nodes PyTorch's autograd puts around F.linear in models/UMNN/made.py:16-27,113-119): g [B, N] fp32 is the gradient w.r.t.
 * the layer's ReLU output `relu_out` (NULL for the last layer: no activation behind it).  In place g <- g . [relu_out > 0], and
 * gb[c] <- sum_r g[r][c] by a two-stage reduction with a fixed order (bit-reproducible; no atomics).  `partial`: row_blocks x N floats
 * of scratch, row_blocks from umnn_made_relu_bwd_bias_row_blocks(B, N). */
int umnn_made_relu_bwd_bias_row_blocks(long long B, int N);
int umnn_made_relu_bwd_bias(float* g, const float* relu_out, long long B, int N, float* partial, int row_blocks, float* gb, void* stream);

/* One step of the PROGRESSIVE conditioner of the sequential sampling walk (csrc/made_step.hip; the reference re-runs the whole MADE
 * before every dimension, UMNNMAF.py:195-231).  With the natural input order a hidden unit of degree m is final once the inputs of
 * degree <= m are, so it is computed once per block and kept in a standing buffer.  The plan holds every hidden layer SORTED BY
 * DEGREE (stable): W[l] [width[l], ldk[l]] the masked fp32 weight (mask * weight, exact zeros kept) permuted on both sides into that
 * order, K axis zero-padded to ldk[l] (a multiple of 4; ldk[0] >= c + d with columns [context | x], ldk[l] >= width[l - 1]); b[l] the
 * permuted bias; W[n_hidden] [d][E][ldk[n_hidden]] / b[n_hidden] [d][E] the output layer regrouped by flow dimension (kept dimensions
 * only for a conditional MADE: c context inputs, d flow dimensions).  steps: HOST table [d][n_hidden + 1][3] of (first new unit, end
 * of new units, input prefix length) per step and layer; the output layer's entry is (0, E, prefix).
 * Step j: for each hidden layer the new units u in [lo, hi):  act[l][b, u] = relu(W[l][u, :prefix] . in[b, :prefix] + b[l][u]) with
 * in = [context | x[:, :j]] for layer 0 and act[l - 1] after it (row stride ldk[l + 1]); then h[b, e d + j] for e < E -- the layout
 * umnn_cc_solve reads.  Never reads x[:, j:] nor a unit outside its prefix.  Exact fp32 products, fp32 accumulation in an order that
 * depends on the prefix only (not on B, the grid or row_tiles: 0 auto | 1 | 2 | 4 tiles of 16 rows per workgroup).
 * LDS bound: at most UMNN_MADE_STEP_MAX_NEW new units per hidden layer in one step (UMNN_EUNSUPPORTED beyond); B == 0 is a no-op. */
#define UMNN_MADE_STEP_MAX_NEW 479
typedef struct umnn_made_plan {
    int n_hidden;
    int d, c, E;
    int width[UMNN_MADE_MAX_LAYERS];
    int ldk[UMNN_MADE_MAX_LAYERS + 1];
    const float* W[UMNN_MADE_MAX_LAYERS + 1];
    const float* b[UMNN_MADE_MAX_LAYERS + 1];
    const int* steps;
} umnn_made_plan;
int umnn_made_step(const umnn_made_plan* plan, int j, const float* context, const float* x, float* const* act, float* h,
                   long long B, int row_tiles, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* UMNN_CC_H */
