"""Float64 truth of the gradient through a flow sample, built once per case on the CPU from code that predates ``inverse``:

  * x64 from ``tests/_inverse_truth.flow_invert64`` over the numpy oracle;
  * the dense per-sample Jacobian J_b = dT/dx of the ``.double()`` model's ``forward`` (generic ATen path, the package's own
    convention dF/dx = f(x)) from ``torch.autograd.functional.jacobian``;
  * lam* = solve(J^T, g_x);  g_theta* = autograd.grad(forward(x64), params, -lam*), the same for the context;
  * kappa = max_b ||J_b^-T||_inf ||J_b^T||_inf, the condition number of that solve.
"""
import copy
import types

import numpy as np
import torch

import umnn_amd
from oracle import cc_oracle as O
from tests import _inverse_truth as T
from tests import _util as U


def make_flow(d, hid, E, n, nb_flow, seed, made_hidden=(32, 32), made_gain=1., cond_in=0):
    """A CPU float32 flow with distinct log-scales per dimension and block; ``made_gain`` multiplies the conditioner's weights."""
    torch.manual_seed(seed)
    m = umnn_amd.UMNNMAFFlow(nb_flow=nb_flow, nb_in=d, hidden_derivative=list(hid), hidden_embedding=list(made_hidden), embedding_s=E,
                             nb_steps=n, solver="CCParallel", cond_in=cond_in).eval()
    with torch.no_grad():
        for i, blk in enumerate(m.nets):
            blk.scaling.copy_(torch.linspace(-0.4, 0.5, d) * (1. - 0.3 * i) if d > 1 else torch.tensor([0.3]))
            if made_gain != 1.:
                for mod in blk.net.made.net:
                    if hasattr(mod, "weight"):
                        mod.weight.mul_(made_gain)
    return m


class _BoundContext:
    """An oracle block whose ``embed(x)`` reads a fixed context: what ``T.flow_invert64`` calls."""

    def __init__(self, blk, context):
        self.net, self.scaling, self._blk, self._context = blk.net, blk.scaling, blk, context

    def embed(self, x):
        return self._blk.embed(x, self._context)


def oracle_blocks(m, context=None):
    sd = {k: v.detach().cpu().numpy() for k, v in m.state_dict().items()}
    made = m.nets[0].net.made
    cond_in = getattr(made, "cond_in", 0)
    blocks = []
    for i in range(len(m.nets)):
        mW, mb, mm = U._seq(sd, f"Flow{i}.net.made.net.", np.float64)
        iW, ib, _ = U._seq(sd, f"Flow{i}.net.parallel_nets.net.", np.float64)
        blk = O.Block(mW, mb, mm, O.Net(iW, ib, O.LEAKY, O.ELU1), sd[f"Flow{i}.scaling"].astype(np.float64), cond_in)
        blocks.append(blk if cond_in == 0 else _BoundContext(blk, np.asarray(context, np.float64)))
    return blocks


def double_of(m):
    m64 = copy.deepcopy(m).to("cpu").double()
    umnn_amd.invalidate_caches(m64)
    return m64


def per_sample_jacobian(fwd, x):
    """J [B, d, d] with J[b, i, j] = d fwd(x)[b, i] / d x[b, j]; the rows of the batch are independent, so the Jacobian of the batch sum
    holds every per-sample one."""
    J = torch.autograd.functional.jacobian(lambda xx: fwd(xx).sum(0), x)        # [d, B, d]
    return J.permute(1, 0, 2).contiguous()


def truth(m, z, g_of_x, context=None, module=None):
    """``m``: the flow (any float dtype, any device); ``module``: the part of it under test -- ``m`` itself (default) or its only block.
    ``z`` [B,d]: float64 targets; ``g_of_x(x64) -> g_x``: the cotangent of the sample.  -> namespace(x, J, g_x, lam, grads {name: tensor
    of ``module.named_parameters()``}, g_context, kappa, kappas)."""
    m64 = double_of(m)
    n = m64.nets[0].nb_steps
    z = torch.as_tensor(z, dtype=torch.float64).cpu()
    ctx = None if context is None else context.detach().cpu().double()
    blocks = oracle_blocks(m64, None if ctx is None else ctx.numpy())
    x_np, mins = T.flow_invert64(blocks, z.numpy(), n)
    x64 = torch.from_numpy(np.ascontiguousarray(x_np))
    target = m64 if module is None or module is m else m64.nets[0]
    assert module is None or module is m or (len(m.nets) == 1 and module is m.nets[0])
    for p in target.parameters():
        p.requires_grad_(True)
    ctx_leaf = None if ctx is None else ctx.clone().requires_grad_(True)
    fwd = lambda xx, c=ctx: target(xx, context=c)
    # The oracle integrates with float64 quadrature tables, the .double() model with the package's float32 tables widened: the two
    # forward maps differ by ~5e-8, and so does x64 from the inverse of the model whose Jacobian is the truth.  A few Newton steps
    # on the model's own forward (dense J, a contraction by the quadrature error of f per step) close that gap to 1e-13.
    assert float((fwd(x64).detach() - z).abs().max()) < 1e-6, "the oracle's inverse, to the difference between the two quadrature tables"
    for _ in range(8):
        res = fwd(x64).detach() - z
        if float(res.abs().max()) < 1e-13:
            break
        x64 = x64 - torch.linalg.solve(per_sample_jacobian(fwd, x64), res.unsqueeze(2)).squeeze(2)
    assert float((fwd(x64).detach() - z).abs().max()) < 1e-12, "x64 is the inverse under the model's own forward"
    J = per_sample_jacobian(fwd, x64)
    g_x = g_of_x(x64).double()
    JT = J.transpose(1, 2)
    lam = torch.linalg.solve(JT, g_x.unsqueeze(2)).squeeze(2)
    names = [k for k, _ in target.named_parameters()]
    params = [p for _, p in target.named_parameters()]
    wanted = params + ([ctx_leaf] if ctx_leaf is not None else [])
    grads = torch.autograd.grad(target(x64, context=ctx_leaf), wanted, -lam, allow_unused=True)
    grads = [torch.zeros_like(p) if g is None else g for g, p in zip(grads, wanted)]
    inf_norm = lambda A: A.abs().sum(2).max(1).values
    kappas = inf_norm(torch.linalg.inv(JT)) * inf_norm(JT)
    # the blocks' own condition numbers, whose product bounds the flow's (each block's J^T is one factor of the flow's, up to flips)
    block_kappas, xi = [], x64
    for blk in m64.nets:
        Jb = per_sample_jacobian(lambda xx, b=blk: b(xx, context=ctx), xi).transpose(1, 2)
        block_kappas.append(float((inf_norm(torch.linalg.inv(Jb)) * inf_norm(Jb)).max()))
        with torch.no_grad():
            xi = torch.flip(blk(xi, context=ctx), [1])
    return types.SimpleNamespace(x=x64, z=z, J=J, g_x=g_x, lam=lam, grads=dict(zip(names, grads[:len(params)])),
                                 g_context=grads[-1] if ctx_leaf is not None else None, kappa=float(kappas.max()),
                                 block_kappas=block_kappas, min_sf=mins)
