"""Host drivers of the sampling direction: what ``invert``, ``inverse`` and the samplers of UMNNMAF / UMNNMAFFlow run.

One record (``Inverted``) is what every block-level walker returns and ``public_value`` is the one place that turns it into the tuple
``invert`` documents; one walk over the blocks of a flow (``walk_blocks``) serves the eager methods, the recorded (torch.compile /
torch.export) forms, ``graphs.GraphedSampler`` and the differentiable ``inverse``; one accumulator (``LogJacSum``) owns the running
log-Jacobian sum; the Newton iteration a kernel refused is driven through ``integral.quadrature_eval`` (it sits beside
``integral.newton_solve``, whose ``host_solve`` / ``aten_solve`` are callers of it too).  The walkers -- ``invert_bracket``, ``invert_newton``,
``invert_jacobi``, ``invert_recorded`` -- are functions of (block, z, context, opts, lj) with ``opts`` an ``Options`` checked once per call.
"""
import os
from typing import NamedTuple

import torch

from . import integral as _I
from .made import ConditionnalMADE
from .nets import single_spec


class Inverted(NamedTuple):
    """What a block-level walker returns.  ``walk_blocks`` returns the flow's: x and the summed lj, with ``info`` / ``status`` / ``move`` as
    lists over the blocks in flow order."""
    x: object
    lj: object = None           # [B]: the running log-Jacobian sum including this block, or None
    info: object = None         # the Jacobi dict, or None
    status: object = None       # the last solve's status words, or None
    move: object = None         # 0-dim device tensor max |x_K - x_{K-1}| / max(1, |x_K|) of the last Jacobi sweep, or None


class Options(NamedTuple):
    """The options of one ``invert`` call (``check`` validates them once)."""
    method: str = "bracket"
    iter: int = 10
    tol: float = 1e-6
    max_iter: int = 64
    sweep_tol: float = 1e-6
    max_sweeps: object = None
    conditioner: str = "full"
    want_info: bool = False
    want_lj: bool = False
    want_move: bool = False     # (graphs.GraphedSampler: the Jacobi walk also computes ``Inverted.move``, without a host read)


def check(opts, who):
    if opts.method not in ("bracket", "newton", "jacobi"):
        raise ValueError(f"umnn_amd: unknown inversion method {opts.method!r}; expected 'bracket', 'newton' or 'jacobi'")
    if opts.conditioner not in ("full", "progressive"):
        raise ValueError(f"umnn_amd: unknown conditioner {opts.conditioner!r}; expected 'full' or 'progressive'")
    if opts.method == "jacobi" and opts.conditioner != "full":
        raise ValueError("umnn_amd: conditioner='progressive' belongs to the dimension-by-dimension walks (method 'newton' or 'bracket'); "
                         "a Jacobi sweep needs the whole conditioner")
    if torch.jit.is_tracing():
        raise RuntimeError(f"umnn_amd: {who}.invert cannot be traced by torch.jit.trace (data-dependent bracket search); "
                           "call it eagerly")
    if opts.want_info and opts.method != "jacobi":
        raise ValueError("umnn_amd: return_info is an option of invert(method='jacobi')")
    if opts.method == "jacobi" and opts.max_sweeps is not None and int(opts.max_sweeps) < 1:
        raise ValueError("umnn_amd: invert(method='jacobi') needs max_sweeps >= 1")


def public_value(out, stacked, want_info, want_lj):
    """The flow's record -> what ``invert`` returns: x, (x, info), (x, log_jac) or (x, info, log_jac); info's entries are lists over the
    blocks in flow order for a UMNNMAFFlow (``stacked``) and the block's own for a single UMNNMAF."""
    res = (out.x,)
    if want_info:
        res += ({k: [inf[k] for inf in out.info] for k in out.info[0]} if stacked else out.info[0],)
    if want_lj:
        res += (out.lj,)
    return res[0] if len(res) == 1 else res


def walk_blocks(blocks, stacked, z, step):
    """The sampling direction over the blocks of a flow: flip once, then for the blocks in reverse flip and ``step(block, z, lj_so_far)
    -> Inverted``; a single UMNNMAF is the one-block walk without flips (``stacked`` False).  Plain control flow over a list (dynamo
    unrolls it) and no no_grad of its own: the flips are differentiable ops for ``inverse``, and each step sets what it needs."""
    recs, lj = [], None
    if stacked:
        z = torch.flip(z, [1])
    for blk in reversed(blocks):
        rec = step(blk, torch.flip(z, [1]) if stacked else z, lj)
        z, lj = rec.x, rec.lj
        recs.insert(0, rec)
    return Inverted(z, lj, [r.info for r in recs], [r.status for r in recs], [r.move for r in recs])


class LogJacSum:
    """The running log-Jacobian row sum of a walk, for one block: ``lj`` [B] so far (None: a fresh sum) plus this block's sum_i
    [log(f(x_i) + 1e-10) + s_i].  In a kernel the sum is contiguous fp32 (a sum that is not starts fresh there and is added in
    torch ops) and the kernels read the fp32 contiguous ``scaling32``; torch ops work in the tensors' dtype on the block's own
    scaling; an entry whose solve ended SOLVE_NONFINITE makes its row's sum NaN."""
    __slots__ = ("lj", "want", "scaling", "scaling32")

    def __init__(self, block, lj, want):
        self.lj, self.want = lj, want
        self.scaling = block.scaling.detach()
        self.scaling32 = self.scaling.float().contiguous()

    def kernel_row(self, B, dev):
        """-> (lj_row, lj_first) of the next ``umnn_cc_solve_lj`` launch; (None, False) when no sum is wanted."""
        if not self.want:
            return None, False
        first = self.lj is None or self.lj.dtype != torch.float32 or not self.lj.is_contiguous()
        return (torch.empty(B, device=dev, dtype=torch.float32) if first else self.lj), first

    def kernel_wrote(self, lj_row, lj_first):
        if lj_first:
            self.lj = lj_row if self.lj is None else self.lj + lj_row

    def add_column(self, j, f_j, status_j):
        """Dimension j from ``integral.newton_solve``'s f(x) and status, both [B,1]."""
        if self.want:
            lj_j = torch.log(f_j[:, 0] + 1e-10) + self.scaling[j].to(f_j.dtype)
            lj_j = torch.where((status_j[:, 0] & _I._lib.SOLVE_NONFINITE) != 0, torch.full_like(lj_j, float("nan")), lj_j)
            self.lj = lj_j if self.lj is None else self.lj + lj_j

    def add_rows(self, fx, x=None):
        """Every dimension from f_x [B,d]: one ``umnn_flow_sample_lj_rows`` launch, or torch ops.  ``x``: the solves' result -- an entry
        that ended non-finite returns x = NaN while its f_x is the last iterate's."""
        if x is not None:
            fx = torch.where(torch.isnan(x), x, fx)
        self.lj = _I.sample_lj_rows(fx.contiguous(), self.scaling32 if fx.dtype == torch.float32 else self.scaling, self.lj)


def _conditional_integral(block, cand, h_j):
    """int_0^cand f(t; h_j) dt for one dimension: cand [R,1], h_j [R,E] -> [R,1]."""
    integrand = block.net.parallel_nets
    spec = single_spec(integrand, "the flow inverse")
    if _I._use_hip(spec, cand):
        return _I.hip_forward(spec, None, cand, h_j, block.nb_steps)[0]
    with torch.no_grad():
        return _I.aten_forward(lambda t, hh: integrand.independant_forward(torch.cat((t, hh), 1)),
                               torch.zeros_like(cand), cand, h_j, block.nb_steps)


def dim_embedding(block, x_inv, context, rows_ok, conditioner="full"):
    """The conditioner pass of the dimension-by-dimension sampling loops -> ``embed(j, widen)``: the embedding h [B, E*d] that
    dimension j is solved under, from ``x_inv``'s current contents.  Dimension j reads E of the E*d embedding entries.  Wide
    unconditional conditioners compute only those columns of their last layer (MADE.raw_rows: for d = 784 that layer is 23 520 rows
    of which 30 are read) into a standing buffer, where ``rows_ok`` (the in-kernel path) and the conditioner allow it; otherwise a
    full pass, with ``widen`` as contiguous fp32 -- exact for a bf16 embedding (set_embedding_dtype, autocast), which the fp32-only
    entry points would misread.
    ``conditioner="progressive"``: ``embed(j, widen)`` is one step of ``made.ProgressiveWalk`` into its standing embedding buffer --
    on the HIP path (``rows_ok``, fp32 x_inv on the weights' device) one ``umnn_made_step`` launch, else the same walk in torch ops."""
    made = block.net.made
    B, d = x_inv.shape
    dev = x_inv.device
    E = made.nout // made.nin
    if conditioner == "progressive":
        plan = made.progressive_plan(dev) if block.net.embedding_dtype in (None, torch.float32) and not torch.is_autocast_enabled() else None
        if plan is None:
            _I._warn_once("progressive-ineligible",
                          "umnn_amd: conditioner='progressive' needs a MADE with the natural input order, one mask, fp32 weights on "
                          "the tensors' device and an fp32 embedding; this one runs conditioner='full'.")
        else:
            use_kernel = bool(rows_ok and x_inv.is_cuda and x_inv.dtype == torch.float32 and x_inv.is_contiguous())
            if rows_ok and x_inv.is_cuda and plan.desc is None:
                _I._warn_once("progressive-torch", "umnn_amd: umnn_made_step does not cover this conditioner (weight dtype, more than 8 "
                              "hidden layers or more new units in one step than its LDS hand-off holds): the progressive walk runs in "
                              "torch ops.")
            walk = plan.walk(x_inv, context, use_kernel)

            def embed_progressive(j, widen):
                h = walk.step(j)
                return h.float().contiguous() if widen and h.dtype != torch.float32 else h
            return embed_progressive
    restrict = (rows_ok and context is None and not isinstance(made, ConditionnalMADE)
                and block.net.embedding_dtype in (None, torch.float32) and os.environ.get("UMNN_INVERT_ROWS", "1") != "0")
    rows_all = (torch.arange(E, device=dev) * d).view(1, E) + torch.arange(d, device=dev).view(d, 1) if restrict else None
    h_buf = None

    def embed(j, widen):
        nonlocal restrict, h_buf
        hj = made.raw_rows(x_inv, rows_all[j]) if restrict else None
        if hj is not None:
            if h_buf is None:
                h_buf = torch.zeros(B, E * d, device=dev)
            h_buf.view(B, E, d)[:, :, j] = hj
            return h_buf
        restrict = False
        h = block.net.make_embeding(x_inv, context)
        return h.float().contiguous() if widen else h
    return embed


def invert_newton(block, z, context, opts, lj=None):
    """``invert(method="newton")`` of one block.  HIP path: d x (conditioner + ONE launch), the whole solve of a dimension inside the
    kernel, writing x_inv[:, j] in place; nets the solve kernels do not cover, host tensors and other dtypes run the same iteration
    from the host (``integral.newton_solve``), one quadrature launch (or ATen quadrature) per iteration -- from the dimension at which
    the kernel refused on, for the rest of the block.
    ``opts.want_lj``: the block's log-Jacobian row sum at x is added to ``lj`` (``LogJacSum``) -- in the solve launch itself
    (``umnn_cc_solve_lj``) on the HIP path, from ``newton_solve``'s f(x) in the tensors' dtype otherwise."""
    B, d = z.shape
    dev = z.device
    integrand = block.net.parallel_nets
    spec = single_spec(integrand, "the flow inverse")
    use_hip = _I._use_hip(spec, z)
    in_kernel = use_hip and z.dtype == torch.float32 and block.nb_steps >= 1 and B > 0 and block.solver in _I.SOLVERS
    with torch.no_grad():
        z = z.contiguous()
        x_inv = torch.zeros(B, d, device=dev, dtype=z.dtype)
        acc = LogJacSum(block, lj, opts.want_lj)
        embed = dim_embedding(block, x_inv, context, in_kernel, opts.conditioner)
        for j in range(block.input_size):
            h = embed(j, in_kernel)             # (umnn_cc_solve reads an fp32 embedding)
            if in_kernel:
                lj_row, lj_first = acc.kernel_row(B, dev)
                if _I.hip_solve(spec, h, z, block.nb_steps, j=j, scaling=acc.scaling32, off_h0=True, lo=-50., hi=50., tol=opts.tol,
                                max_iter=opts.max_iter, x_out=x_inv, want_info=False, lj_row=lj_row, lj_first=lj_first) is not None:
                    acc.kernel_wrote(lj_row, lj_first)
                    continue
                in_kernel = False
            h_j = h.view(B, h.shape[1] // d, d)[:, :, j].to(z.dtype).contiguous()          # [B,E]; row 0 doubles as the offset
            eval_fn = _I.quadrature_eval(spec, integrand, h_j, block.nb_steps, use_hip, column=True)
            x_j, f_j, st_j = _I.newton_solve(eval_fn, z[:, [j]], torch.exp(block.scaling[j]).to(z.dtype), h_j[:, [0]], -50., 50.,
                                             opts.tol, opts.max_iter)
            x_inv[:, j] = x_j[:, 0]
            acc.add_column(j, f_j, st_j)
    return Inverted(x_inv, acc.lj)


def _jacobi_info(sweeps, converged, status, max_evals):
    return {"sweeps": sweeps, "converged": converged, "status": status, "max_evals": max_evals}


def invert_empty(block, z, context, opts, lj=None):
    """The walkers' result for an empty batch, which their generic loops cannot shape an embedding for: empty tensors of the walks'
    dtypes and the info of a Jacobi walk that had nothing to sweep."""
    bracket = opts.method == "bracket"
    if lj is None:
        lj = torch.zeros(0, device=z.device, dtype=block.pi.dtype if bracket else z.dtype)
    info = _jacobi_info(0, True, torch.zeros(z.shape, device=z.device, dtype=torch.int32), []) if opts.want_info else None
    return Inverted(torch.zeros_like(z, dtype=torch.float32 if bracket else z.dtype), lj, info)


def invert_jacobi(block, z, context, opts, lj=None):
    """``invert(method="jacobi")`` of one block: x <- 0; repeat { h <- conditioner(x); x_i <- solve_i(z_i; h) for EVERY i }.  The
    conditioner is autoregressive, so dimension i is final once x_<i are: after sweep t the first t dimensions hold the sequential
    answer, d sweeps reproduce ``method="newton"``, and a fixed point is the inverse.  HIP path: per sweep one conditioner pass and ONE
    launch over the B d rows (``umnn_cc_solve_block``), every sweep after the first warm-started from the previous x; host tensors,
    other dtypes and nets the solve kernels do not cover run the same sweeps through ``integral.newton_solve`` over [B, d].
    Stops when max |x_new - x| / max(1, |x_new|) <= ``sweep_tol`` (one scalar device-to-host read per sweep; ``sweep_tol`` = 0: no
    test and no read), in any case after ``max_sweeps`` sweeps (default d).  info (``opts.want_info``) = {"sweeps", "converged": the
    test was met or d sweeps ran, "status": the last sweep's status words [B,d], "max_evals": per sweep}.
    ``opts.want_lj``: the sweeps also write their f_x (the same launch) and the last sweep's row sums of log(f_x + 1e-10) + s are
    added to ``lj`` by one ``umnn_flow_sample_lj_rows`` launch -- the last sweep solved every dimension under the embedding of
    x_{K-1}, so the sum is the block's log-Jacobian at the returned x to the same order as x itself is the inverse."""
    B, d = z.shape
    dev = z.device
    integrand = block.net.parallel_nets
    spec = single_spec(integrand, "the flow inverse")
    use_hip = _I._use_hip(spec, z) and block.nb_steps >= 1 and block.solver in _I.SOLVERS and z.dtype == torch.float32
    in_kernel = use_hip and B > 0
    max_sweeps = d if opts.max_sweeps is None else int(opts.max_sweeps)
    want_info, sweep_tol = opts.want_info, opts.sweep_tol
    with torch.no_grad():
        z = z.contiguous()
        x = torch.zeros(B, d, device=dev, dtype=z.dtype)
        acc = LogJacSum(block, lj, opts.want_lj)
        sweeps, met, status, evals, x_prev, fx = 0, False, None, [], x, None
        for sweep in range(max_sweeps):
            h = block.net.make_embeding(x, context)
            x_init = x if sweep > 0 else None
            out = None
            if in_kernel:
                # (umnn_cc_solve_block reads an fp32 embedding; widening bf16 is exact)
                out = _I.hip_solve_block(spec, h.float().contiguous(), z, block.nb_steps, scaling=acc.scaling32, off_h0=True, x_init=x_init,
                                         lo=-50., hi=50., tol=opts.tol, max_iter=opts.max_iter, want_info=want_info or opts.want_lj)
                in_kernel = out is not None
            if out is None:
                eval_fn = _I.quadrature_eval(spec, integrand, h if use_hip else h.to(z.dtype), block.nb_steps, use_hip)
                off = h.view(B, h.shape[1] // d, d)[:, 0, :].to(z.dtype)
                out = _I.newton_solve(eval_fn, z, torch.exp(block.scaling).to(z.dtype).unsqueeze(0), off, -50., 50., opts.tol, opts.max_iter,
                                      x_init=x_init)
            x_new, fx, status = out
            sweeps += 1
            if want_info:
                evals.append((status & _I._lib.SOLVE_EVALS_MASK).max() if B > 0 else torch.zeros((), dtype=torch.int32, device=dev))
            if sweep_tol > 0:
                moved = (x_new - x).abs() > sweep_tol * x_new.abs().clamp(min=1.)      # (a NaN row never counts as moving)
                met = not bool(moved.any())
            x_prev, x = x, x_new
            if met:
                break
        move = ((x - x_prev).abs() / x.abs().clamp(min=1.)).max() if opts.want_move else None
        if opts.want_lj:
            acc.add_rows(fx, x)
    info = _jacobi_info(sweeps, bool(met or sweeps >= d), status, [int(e) for e in torch.stack(evals).tolist()]) if want_info else None
    return Inverted(x, acc.lj, info, status, move)


def invert_recorded(block, z, context, opts, lj=None):
    """One block of ``invert`` as a graph records it (under the caller's no_grad): "newton", or "jacobi" with its fixed sweep count K =
    ``opts.max_sweeps``.  info (jacobi, ``opts.want_info``) = {"sweeps": K, the last sweep's "status", "last_move": ``Inverted.move``, which
    the caller may test afterwards (NaN when a row ended non-finite)}.  ``opts.want_lj``: the row sum of log(f_x + 1e-10) + s, composed
    in torch ops from the f_x the solve ops return (the newton form adds one column per step, the jacobi form sums the last sweep's
    f_x), is added to ``lj``.
    The conditioner runs in its graph-mode composition with every mask product formed ONCE for the whole block inversion; scale
    and offset are folded into the target by torch ops, t = z exp(-s) - h[:, 0, :], as ``MonotonicNN.inverse`` does.
    "newton": input_size steps of conditioner + ``umnn::cc_solve`` on the [B, 1] column -- the loop unrolls at trace time, so this is
    for small d; wide blocks record "jacobi": K x (conditioner + ``umnn::cc_solve_block`` warm-started from the previous sweep), no
    test between them."""
    B = z.shape[0]
    d = block.input_size
    net_args = _I.spec_args(_I._hip_spec(block.net.parallel_nets, z, True))
    weights = block.net.made.graph_weights()
    n, tol, max_iter = int(block.nb_steps), float(opts.tol), int(opts.max_iter)
    target = z * torch.exp(-block.scaling.detach().float()).unsqueeze(0)
    x = torch.zeros_like(z)
    s = block.scaling.detach().float()
    x_prev, status, move, info = x, None, None, None
    if opts.method == "newton":
        fxs = []
        for j in range(d):
            h_j = block.net.graph_embedding(x, context, weights).view(B, -1, d)[:, :, j]       # [B,E]; row 0 doubles as the offset
            x_j, fx_j, _ = torch.ops.umnn.cc_solve(target[:, j:j + 1] - h_j[:, :1].float(), h_j, *net_args, n, -50., 50., tol, max_iter)
            x = torch.cat((x[:, :j], x_j, x[:, j + 1:]), 1)
            fxs.append(fx_j)
        fx = torch.cat(fxs, 1) if opts.want_lj else None
    else:
        for sweep in range(int(opts.max_sweeps)):
            h = block.net.graph_embedding(x, context, weights)
            t = target - h.view(B, -1, d)[:, 0, :].float()
            x_new, fx, status = torch.ops.umnn.cc_solve_block(t, h, x if sweep > 0 else None, *net_args, n, -50., 50., tol, max_iter)
            x_prev, x = x, x_new
        move = ((x - x_prev).abs() / x.abs().clamp(min=1.)).max()
        if opts.want_info:
            info = {"sweeps": int(opts.max_sweeps), "status": status, "last_move": move}
    if opts.want_lj:
        lj_blk = (torch.log(fx + 1e-10) + s.unsqueeze(0)).sum(1)
        lj = lj_blk if lj is None else lj + lj_blk
    return Inverted(x, lj, info, status, move)


def bracket_search(block, z, iter, context, conditioner):
    """The reference's bracket search of one block -> (x, h): h the embedding the last dimension was searched under."""
    K = 10
    B, d = z.shape
    dev = z.device
    spec = single_spec(block.net.parallel_nets, "the flow inverse")
    if (_I._use_hip(spec, z) and z.dtype == torch.float32 and block.nb_steps >= 1 and iter >= 1 and B > 0
            and block.solver in _I.SOLVERS):
        # d x (conditioner + ONE launch): the whole 10-way / `iter`-round search of a dimension runs inside the kernel
        with torch.no_grad():
            z = z.contiguous()
            x_inv = torch.zeros(B, d, device=dev)
            scaling = block.scaling.detach().float().contiguous()
            done = True
            embed = dim_embedding(block, x_inv, context, True, conditioner)
            for j in range(block.input_size):
                h = embed(j, True)              # (umnn_flow_invert_dim reads an fp32 embedding: it has no umnn_io descriptor)
                if not _I.hip_invert_dim(spec, h, z, scaling, block.nb_steps, j, iter, x_inv):
                    done = False
                    break
        if done:
            return x_inv, h
    frac = torch.linspace(0., 1., K, device=dev).view(K, 1)
    x_inv = torch.zeros(B, d, device=dev)
    scale = torch.exp(block.scaling)
    rows = torch.arange(B, device=dev)
    with torch.no_grad():
        embed = dim_embedding(block, x_inv, context, False, conditioner) if conditioner != "full" else None
        for j in range(block.input_size):
            h = block.net.make_embeding(x_inv, context) if embed is None else embed(j, False)
            h3 = h.view(B, h.shape[1] // d, d)
            h_j = h3[:, :, j]                                   # [B,E]; row 0 doubles as the offset
            offset = h_j[:, 0]
            h_rep = h_j.unsqueeze(0).expand(K, -1, -1).reshape(K * B, -1)
            left = torch.full((B,), -50., device=dev)
            right = torch.full((B,), 50., device=dev)
            best = torch.zeros(B, device=dev)
            for _ in range(iter):
                cand = frac * (right - left).unsqueeze(0) + left.unsqueeze(0)          # [K,B]
                F = _conditional_integral(block, cand.reshape(-1, 1), h_rep).view(K, B)
                z_est = scale[j] * (offset.unsqueeze(0) + F)
                m = torch.abs(z_est - z[:, j].unsqueeze(0)).argmin(0)                  # [B]
                below = z_est[m, rows] < z[:, j]
                lo = cand[(m - 1).clamp(min=0), rows]
                hi = cand[(m + 1).clamp(max=K - 1), rows]
                best = cand[m, rows]
                left = torch.where(below, best, lo)
                right = torch.where(below, hi, best)
            x_inv[:, j] = best
    return x_inv, h


def invert_bracket(block, z, context, opts, lj=None):
    """``invert(method="bracket")`` of one block: the search (fp32 whatever the block's dtype is).  ``opts.want_lj``: the search never
    evaluates f(x), so this is the one method that pays a pass for the log-Jacobian -- one forward launch of the block's integrand at
    the result (f(x) is node 0 of a one-step quadrature, as in ``compute_log_jac``) under the embedding the search's last dimension
    left, which is the embedding of the result (the conditioner is autoregressive: every column was final when it was computed), so
    no conditioner pass more; its row sums are added to ``lj``."""
    x, h = bracket_search(block, z, opts.iter, context, opts.conditioner)
    if not opts.want_lj:
        return Inverted(x, lj)
    with torch.no_grad():
        integrand = block.net.parallel_nets
        spec = _I._hip_spec(integrand, x)
        if spec is not None and h.is_cuda:
            fx = _I.cc_forward_jac(spec, integrand, None, x, h, 1, True)[1]
        else:
            dt = block.scaling.dtype
            fx = integrand(x.to(dt), h.to(dt))
        acc = LogJacSum(block, lj, True)
        acc.add_rows(fx)
    return Inverted(x, acc.lj)


_WALKERS = {"bracket": invert_bracket, "newton": invert_newton, "jacobi": invert_jacobi}


def run(blocks, stacked, z, context, opts, empty=False):
    """The eager walk of ``invert`` with checked options -> the flow's ``Inverted`` (``invert`` and ``graphs.GraphedSampler``)."""
    walker = invert_empty if empty else _WALKERS[opts.method]
    return walk_blocks(blocks, stacked, z, lambda blk, zz, lj: walker(blk, zz, context, opts, lj))


def _recordable(blocks, z, opts):
    """This ``invert`` call, met while torch.compile / torch.export trace, is one the graph can hold: "newton", or "jacobi" with a
    fixed sweep count (``sweep_tol`` = 0 and ``max_sweeps`` given: no host read decides anything), the full conditioner (the progressive
    walk is an eager call, like "bracket"), fp32 z and every block on the HIP path (``integral._hip_spec``)."""
    if opts.conditioner != "full" or opts.method == "bracket" or (opts.method == "jacobi" and (opts.sweep_tol != 0 or opts.max_sweeps is None)):
        return False
    if len(blocks) == 0 or z.dim() != 2 or z.dtype != torch.float32:
        return False
    return all(blk.solver in _I.SOLVERS and blk.nb_steps >= 1 and _I._hip_spec(blk.net.parallel_nets, z, True) is not None
               for blk in blocks)


def invert(blocks, stacked, who, z, context, opts):
    """``invert`` of UMNNMAF (``blocks`` = [block], ``stacked`` False) and UMNNMAFFlow (the blocks in flow order): checks the options and
    walks the blocks with the method's walker.  While torch.compile / torch.export trace, "newton" and fixed-sweep "jacobi" on the HIP
    path are recorded (``invert_recorded``); every other call there is an eager call the graph breaks at, and torch.jit.trace raises."""
    check(opts, who)
    compiling = torch.compiler.is_compiling()
    if compiling and _recordable(blocks, z, opts):
        with torch.no_grad():
            out = walk_blocks(blocks, stacked, z, lambda blk, zz, lj: invert_recorded(blk, zz, context, opts, lj))
    else:
        # (applied here, not as a decorator: torch.compiler.disable imports torch._dynamo, ~1 s at every package import)
        fn = torch.compiler.disable(run) if compiling else run
        out = fn(blocks, stacked, z, context, opts, opts.want_lj and z.shape[0] == 0 and not compiling)
    return public_value(out, stacked, opts.want_info, opts.want_lj)


def base_noise(pi, block, n, generator=None):
    """z ~ N(0, I), [n, d] on the device of the model's ``pi`` (drawn on the generator's own device when one is given)."""
    dev = pi.device
    z = torch.randn(int(n), block.input_size, generator=generator, dtype=block.scaling.dtype, device=dev if generator is None else generator.device)
    return z.to(dev)


def sample_and_log_prob(flow, block, n, context, generator, solve_opts):
    """``sample_and_log_prob`` of UMNNMAF and UMNNMAFFlow: noise, ``invert(..., return_log_jac=True)``, the Gaussian term."""
    solve_opts.setdefault("method", "newton")
    if solve_opts.pop("return_info", False):
        raise ValueError("umnn_amd: sample_and_log_prob returns (x, log_prob); ask invert(..., return_info=True, return_log_jac=True) for the info")
    with torch.no_grad():
        z = base_noise(flow.pi, block, n, generator)
        x, lj = flow.invert(z, context=context, return_log_jac=True, **solve_opts)
        return x, _I.sample_ll(z.contiguous(), lj.contiguous(), flow.pi)
