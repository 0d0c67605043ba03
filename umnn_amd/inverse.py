"""Differentiable sampling: x = T^-1(z; theta, context) of a UMNN-MAF block or flow with gradients to z, theta and the context.

The forward is the existing no-grad solve (``UMNNMAF.invert(method="newton" | "jacobi")``).  The gradient is the implicit one.  With
z = T(x) the block's forward map and J = dT/dx in the block's own dimension order, a cotangent g_x of x gives

    g_z = lam,    g_theta = -(dT/dtheta)^T lam,    g_context = -(dT/dcontext)^T lam,    where  J^T lam = g_x.

The conditioner is autoregressive, so J is lower triangular with diagonal D_i = exp(s_i) f(x_i; h_i) = exp(log_jac_i) (up to the
1e-10 inside the log).  J^T lam = g_x is solved by the Jacobi iteration that mirrors ``invert(method="jacobi")``:

    lam^0 = g_x / D,        lam^{k+1} = lam^k + (g_x - J^T lam^k) / D.

The iteration matrix I - D^-1 J^T is strictly upper triangular, hence nilpotent: component d-1 is final in lam^0, every sweep
finalises one more, d sweeps are exact and a weakly coupled block needs a few.  One sweep is ONE VJP of the block with respect to x --
the training backward without its parameter gradients (``FlowBlockTransform.backward`` -> ``umnn_cc_backward`` with dtheta = NULL ->
the conditioner chain without its weight GEMMs) -- plus one elementwise launch (``umnn_flow_adjoint_update``).

The Jacobian is the package's (and the reference's) own: dF/dx = f(x), the Leibniz term, not the derivative of the quadrature sum.
A finite difference of ``invert`` therefore differs from these gradients by the quadrature error of f (0.5 % at 20 steps on the test
block); the dense float64 implicit solve of the tests is the truth, a finite difference is not.
"""
import torch
from torch.autograd.function import once_differentiable
from torch.func import functional_call

from . import integral as _I
from .sampling import Inverted, walk_blocks

METHODS = ("newton", "jacobi")


class _LogJacBis(torch.nn.Module):
    """``block.compute_log_jac_bis`` as a ``forward``, which is what ``functional_call`` calls."""

    def __init__(self, block):
        super().__init__()
        self.block = block

    def forward(self, x, context):
        return self.block.compute_log_jac_bis(x, context)


def _block_graph(block, names, params, x, context):
    """(z, log_jac) = block.compute_log_jac_bis(x, context) with ``params`` standing in for the block's parameters: the graph reaches
    exactly the tensors among x, context and params that require grad, and the module's own parameters are not touched."""
    with torch.enable_grad():
        return functional_call(_LogJacBis(block), {"block." + n: p for n, p in zip(names, params)}, (x, context))


class FlowBlockInverse(torch.autograd.Function):
    """x = block^-1(z) as one autograd node.

        FlowBlockInverse.apply(z, context, block, opts, record, *block.parameters())  ->  x

    ``opts``: dict(method, tol, max_iter, sweep_tol, max_sweeps, adj_tol, max_adj_sweeps); ``record``: None or (info, i) -- the forward
    stores the Jacobi solve's info in info["solve"][i], the backward {"sweeps", "vjps", "flags"} in info["adjoint"][i]: "sweeps" counts
    the updates lam needed -- the k of the first lam^k that met the test, or the cap --, "vjps" the block VJPs run (one more than
    "sweeps" when the test ended the loop: the VJP that found lam^k converged), "flags" the last flag word read.
    Backward: the adjoint Jacobi sweeps of the module docstring on a graph whose parameters and context are detached (no parameter
    gradient work inside a sweep), the flag word read once per sweep (4 bytes) unless adj_tol = 0; then one VJP of a second graph,
    x detached, with cotangent -lam for the parameters (``scaling`` included when it requires grad) and the context."""

    @staticmethod
    def forward(ctx, z, context, block, opts, record, *params):
        method = opts["method"]
        with torch.no_grad():
            out = block.invert(z, context=context, method=method, tol=opts["tol"], max_iter=opts["max_iter"],
                               sweep_tol=opts["sweep_tol"], max_sweeps=opts["max_sweeps"], return_info=method == "jacobi")
        x, solve_info = out if method == "jacobi" else (out, None)
        if record is not None:
            record[0]["solve"][record[1]] = solve_info
        ctx.block, ctx.opts, ctx.record = block, opts, record
        ctx.names = [n for n, _ in block.named_parameters()]
        ctx.force_generic = getattr(_I._state, "force_generic", False)     # (thread-local; the backward runs on autograd's threads)
        ctx.save_for_backward(x, context, *params)
        return x

    @staticmethod
    @once_differentiable
    def backward(ctx, g_x):
        x, context, *params = ctx.saved_tensors
        block, opts, nig = ctx.block, ctx.opts, ctx.needs_input_grad
        d = x.shape[1]
        adj_tol = float(opts["adj_tol"])
        max_sweeps = d if opts["max_adj_sweeps"] is None else int(opts["max_adj_sweeps"])
        embedding = block.net.m_embeding
        old_generic = getattr(_I._state, "force_generic", False)
        _I._state.force_generic = ctx.force_generic
        try:
            frozen_ctx = None if context is None else context.detach()
            x_t = x.detach().requires_grad_()
            z_t, log_jac = _block_graph(block, ctx.names, [p.detach() for p in params], x_t, frozen_ctx)
            log_jac = log_jac.detach().contiguous()
            g = g_x.contiguous()
            lam = g * torch.exp(-log_jac)
            flags = torch.zeros(1, dtype=torch.int32, device=x.device)
            sweeps, vjps, word = 0, 0, None
            for _ in range(max_sweeps):
                (r,) = torch.autograd.grad(z_t, x_t, lam, retain_graph=True)
                if adj_tol > 0 and vjps > 0:
                    flags.zero_()
                _I.flow_adjoint_update(g, r.contiguous(), log_jac, lam, adj_tol, flags, out=lam)
                vjps += 1
                if adj_tol > 0:
                    word = int(flags.item())
                    if not word & 1:        # lam already met the test before this update (which moved it by less than the tolerance)
                        break
                sweeps += 1
            del z_t, x_t
            if ctx.record is not None:
                ctx.record[0]["adjoint"][ctx.record[1]] = {"sweeps": sweeps, "vjps": vjps, "flags": word}
            grads = [None] * len(params)
            g_context = None
            if nig[1] or any(nig[5:]):
                leaves = [p.detach().requires_grad_(bool(need)) for p, need in zip(params, nig[5:])]
                leaf_ctx = None if context is None else context.detach().requires_grad_(bool(nig[1]))
                z_p, _ = _block_graph(block, ctx.names, leaves, x.detach(), leaf_ctx)
                wanted = [p for p in leaves if p.requires_grad] + ([leaf_ctx] if nig[1] else [])
                out = list(torch.autograd.grad(z_p, wanted, -lam, allow_unused=True))
                if nig[1]:
                    g_context = out.pop()
                    if g_context is None:
                        g_context = torch.zeros_like(context)
                it = iter(out)
                grads = [next(it) if p.requires_grad else None for p in leaves]
        finally:
            _I._state.force_generic = old_generic
            block.net.m_embeding = embedding
        return (lam if nig[0] else None, g_context, None, None, None, *grads)


def _inverse(blocks, stacked, z, context, opts, return_info):
    nb = len(blocks)
    info = {"method": opts["method"], "solve": [None] * nb, "adjoint": [None] * nb}
    def step(numbered, z, lj):
        i, block = numbered
        return Inverted(FlowBlockInverse.apply(z, context, block, opts, (info, i), *block.parameters()))
    x = walk_blocks(list(enumerate(blocks)), stacked, z, step).x       # (the walk of ``invert``; its flips are differentiable ops here)
    return (x, info) if return_info else x


def inverse(blocks, stacked, who, z, context=None, method="newton", tol=1e-6, max_iter=64, sweep_tol=1e-6, max_sweeps=None,
            adj_tol=1e-6, max_adj_sweeps=None, return_info=False):
    """What ``UMNNMAF.inverse`` (one block, ``stacked`` False) and ``UMNNMAFFlow.inverse`` (the blocks in flow order, with the
    dimension reversal between them) share.  Eager only, like ``invert``: compiled callers get an eager call, torch.jit.trace raises."""
    if method not in METHODS:
        raise ValueError(f"umnn_amd: {who} solves with method 'newton' or 'jacobi', not {method!r} (the bracket search of invert() "
                         "stops at its grid, not at a residual: the implicit gradient needs a solution of T(x) = z)")
    if max_adj_sweeps is not None and int(max_adj_sweeps) < 0:
        raise ValueError(f"umnn_amd: {who} needs max_adj_sweeps >= 0")
    if not adj_tol >= 0:
        raise ValueError(f"umnn_amd: {who} needs adj_tol >= 0")
    if torch.jit.is_tracing():
        raise RuntimeError(f"umnn_amd: {who} cannot be traced by torch.jit.trace (data-dependent solve and sweep counts); call it eagerly")
    opts = dict(method=method, tol=tol, max_iter=max_iter, sweep_tol=sweep_tol, max_sweeps=max_sweeps, adj_tol=adj_tol,
                max_adj_sweeps=max_adj_sweeps)
    fn = torch.compiler.disable(_inverse) if torch.compiler.is_compiling() else _inverse
    return fn(list(blocks), stacked, z, context, opts, return_info)
