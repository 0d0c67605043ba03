"""``UMNNMAF.inverse`` / ``UMNNMAFFlow.inverse``, ``sample``, ``rsample`` and ``log_prob`` without a GPU: float64 on the generic ATen path.

Truth (tests/_flow_inverse_truth.py): x64 from the float64 oracle's inverse, the dense per-sample Jacobian of the ``.double()`` model's
``forward``, lam* = solve(J^T, g_x), g_theta* = autograd.grad(forward(x64), params, -lam*).  The block is d = 5, B = 4, n = 20, integrand
[40, 33], E = 3, MADE [32, 32] with its weights times 3 and distinct log-scales.  Gradients are compared by max |a - b| / max |b|
(``U.scaled_err``) against 1e-9; measured 1e-15 (g_z) to 3e-13 (parameters); the margin covers the 1e-10 inside log_jac, which makes
D = exp(log_jac) differ from J's diagonal.

The solve runs with tol = 1e-13 here, not its default 1e-6: the gradient is taken AT the solution, so an x that is 1e-6 off moves every
gradient by as much, and the 1e-9 of these tests is about the adjoint, not about the solve.  For the same reason the truth's x64 is
polished on the model's own forward: the oracle integrates with float64 tables, the package with float32 ones (5e-8 apart)."""
import ctypes

import pytest
import torch

import umnn_amd
from tests import _flow_inverse_truth as FT
from tests import _util as U
from umnn_amd import _lib, integral

D, B, N = 5, 4, 20
TIGHT = dict(tol=1e-13, max_iter=200)
BOUND = 1e-9

_CASES = {}


def _case(kind):
    """Model, inputs and truth of one configuration, built once and shared; nothing in it is modified afterwards (gradients are taken
    with ``torch.autograd.grad``, which leaves ``.grad`` alone)."""
    if kind not in _CASES:
        nb_flow, cond = {"block": (1, 0), "flow2": (2, 0), "cond": (2, 3)}[kind]
        m = FT.make_flow(D, [40, 33], 3, N, nb_flow, seed=1 + nb_flow + cond, made_gain=3., cond_in=cond).double()
        umnn_amd.invalidate_caches(m)
        g = torch.Generator().manual_seed(7 + nb_flow + cond)
        x0 = 1.5 * torch.randn(B, D, generator=g, dtype=torch.float64)
        G = torch.randn(B, D, generator=g, dtype=torch.float64)
        ctx = torch.randn(B, cond, generator=g, dtype=torch.float64) if cond else None
        module = m.nets[0] if kind == "block" else m
        for p in module.parameters():
            p.requires_grad_(True)                        # (``scaling`` included: the reference freezes it, a user may not)
        with torch.no_grad():
            z = module(x0, context=ctx)
        tr = FT.truth(m, z, lambda x: G, context=ctx, module=module)
        assert float((tr.x - x0).abs().max()) < 1e-9
        _CASES[kind] = (m, module, z, G, ctx, tr)
    return _CASES[kind]


def _grads(module, z, G, ctx, **kw):
    """-> (x, g_z, {name: g_theta}, g_context, info) of loss = sum(x * G)."""
    zz = z.clone().requires_grad_()
    cc = None if ctx is None else ctx.clone().requires_grad_()
    x, info = module.inverse(zz, context=cc, return_info=True, **kw)
    names = [k for k, _ in module.named_parameters()]
    out = torch.autograd.grad((x * G).sum(), [zz] + ([cc] if cc is not None else []) + list(module.parameters()))
    return x.detach(), out[0], dict(zip(names, out[1 + (cc is not None):])), (out[1] if cc is not None else None), info


def _worst(tag, tr, g_z, g_theta, g_ctx=None):
    errs = {"g_z": U.scaled_err(g_z.numpy(), tr.lam.numpy())}
    errs.update({k: U.scaled_err(v.numpy(), tr.grads[k].numpy()) for k, v in g_theta.items()})
    if g_ctx is not None:
        errs["g_context"] = U.scaled_err(g_ctx.numpy(), tr.g_context.numpy())
    worst = max(errs, key=errs.get)
    print(f"{tag}: g_z {errs['g_z']:.2e}, worst {worst} {errs[worst]:.2e} of {len(errs)} gradients (bound {BOUND:.0e})")
    return errs


def test_block_gradients_against_the_dense_solve():
    m, blk, z, G, ctx, tr = _case("block")
    before = blk.net.m_embeding
    flags = {k: p.requires_grad for k, p in blk.named_parameters()}
    x, g_z, g_theta, _, info = _grads(blk, z, G, None, adj_tol=0., **TIGHT)
    assert umnn_amd.path_taken() == "aten"
    assert float((x - tr.x).abs().max()) < 1e-11
    assert info["adjoint"] == [{"sweeps": D, "vjps": D, "flags": None}] and info["solve"] == [None] and info["method"] == "newton"
    errs = _worst("block, d sweeps", tr, g_z, g_theta)
    assert set(g_theta) == set(tr.grads) and "scaling" in g_theta and len(g_theta) == 13
    assert max(errs.values()) <= BOUND, errs
    assert float(tr.grads["scaling"].abs().max()) > 1e-3 and float(tr.grads["net.made.net.0.weight"].abs().max()) > 1e-3
    # module state: the parameters' flags are untouched and the cached embedding is the one the forward's solve left
    assert {k: p.requires_grad for k, p in blk.named_parameters()} == flags
    assert blk.net.m_embeding is not before
    zz = z.clone().requires_grad_()
    xx = blk.inverse(zz, **TIGHT)
    emb = blk.net.m_embeding
    (xx * G).sum().backward(inputs=[zz])
    assert blk.net.m_embeding is emb


def test_frozen_scaling_and_frozen_parameters_get_no_gradient():
    m, blk, z, G, ctx, tr = _case("block")
    blk.scaling.requires_grad_(False)
    blk.net.made.net[2].weight.requires_grad_(False)
    try:
        zz = z.clone().requires_grad_()
        x = blk.inverse(zz, adj_tol=0., **TIGHT)
        wanted = {k: p for k, p in blk.named_parameters() if p.requires_grad}
        out = torch.autograd.grad((x * G).sum(), [zz] + list(wanted.values()))
    finally:
        blk.scaling.requires_grad_(True)
        blk.net.made.net[2].weight.requires_grad_(True)
    assert len(wanted) == 11
    errs = _worst("block, two frozen parameters", tr, out[0], dict(zip(wanted, out[1:])))
    assert max(errs.values()) <= BOUND, errs
    # nothing requires grad: no graph at all
    with torch.no_grad():
        assert not blk.inverse(z, **TIGHT).requires_grad
    for p in blk.parameters():
        p.requires_grad_(False)
    try:
        assert not blk.inverse(z, **TIGHT).requires_grad
    finally:
        for p in blk.parameters():
            p.requires_grad_(True)


def test_every_sweep_finalises_one_more_component():
    m, blk, z, G, ctx, tr = _case("block")
    full = _grads(blk, z, G, None, adj_tol=0., **TIGHT)[1]
    moved = []
    for k in range(D):
        _, g_z, _, _, info = _grads(blk, z, G, None, adj_tol=0., max_adj_sweeps=k, **TIGHT)
        assert info["adjoint"][0]["sweeps"] == k
        diff = (g_z - full).abs().max(0).values
        moved.append(float(diff.max()))
        assert float(diff[D - 1 - k:].max()) <= 1e-8, (k, diff.tolist())
    print("max |lam^k - lam^d| for k = 0..d-1:", " ".join(f"{v:.1e}" for v in moved))
    assert moved[0] > 1e-2 and moved[2] > 1e-6, "the block is coupled: the early iterates are not the answer"
    assert moved[D - 1] <= 1e-8, "d - 1 sweeps are already exact: J is triangular"


def test_early_stop():
    m, blk, z, G, ctx, tr = _case("block")
    _, g_z, g_theta, _, info = _grads(blk, z, G, None, adj_tol=1e-6, **TIGHT)
    rec = info["adjoint"][0]
    res = (G - torch.einsum("bij,bi->bj", tr.J, g_z)).abs() / G.abs().clamp(min=1.)
    print(f"adj_tol 1e-6: {rec}, final residual {float(res.max()):.2e}")
    assert rec["sweeps"] < D and rec["vjps"] == rec["sweeps"] + 1 and rec["flags"] == 0
    assert float(res.max()) <= 1e-6
    # a loose tolerance stops earlier and says so; the cap wins over the test, and then bit 0 is still set
    _, g_loose, _, _, info_loose = _grads(blk, z, G, None, adj_tol=1e-1, **TIGHT)
    assert info_loose["adjoint"][0]["sweeps"] < rec["sweeps"]
    res = (G - torch.einsum("bij,bi->bj", tr.J, g_loose)).abs() / G.abs().clamp(min=1.)
    assert 1e-6 < float(res.max()) <= 1e-1
    _, _, _, _, info_cap = _grads(blk, z, G, None, adj_tol=1e-6, max_adj_sweeps=2, **TIGHT)
    assert info_cap["adjoint"][0] == {"sweeps": 2, "vjps": 2, "flags": 1}


@pytest.mark.parametrize("kind", ["flow2", "cond"])
def test_flow_gradients_against_the_dense_solve(kind):
    m, flow, z, G, ctx, tr = _case(kind)
    x, g_z, g_theta, g_ctx, info = _grads(flow, z, G, ctx, adj_tol=0., **TIGHT)
    assert float((x - tr.x).abs().max()) < 1e-11
    assert [r["sweeps"] for r in info["adjoint"]] == [D, D]
    errs = _worst(kind, tr, g_z, g_theta, g_ctx)
    assert max(errs.values()) <= BOUND, errs
    assert (g_ctx is None) == (kind == "flow2")
    if kind == "cond":
        assert float(tr.g_context.abs().max()) > 1e-3
    # early stop through the stack: per-block records in flow order, the same gradients to the tolerance's order
    _, g_z2, _, _, info2 = _grads(flow, z, G, ctx, **TIGHT)
    assert all(r["sweeps"] < D and r["flags"] == 0 for r in info2["adjoint"])
    assert U.scaled_err(g_z2.numpy(), tr.lam.numpy()) < 1e-4


@pytest.mark.parametrize("kind", ["block", "cond"])
def test_jacobi_solve_gives_the_same_gradients(kind):
    m, module, z, G, ctx, tr = _case(kind)
    x, g_z, g_theta, g_ctx, info = _grads(module, z, G, ctx, method="jacobi", sweep_tol=0., adj_tol=0., **TIGHT)
    assert info["method"] == "jacobi" and all(s["sweeps"] == D for s in info["solve"])
    errs = _worst(f"{kind}, jacobi solve", tr, g_z, g_theta, g_ctx)
    assert max(errs.values()) <= BOUND, errs
    ref = _grads(module, z, G, ctx, adj_tol=0., **TIGHT)
    assert U.scaled_err(g_z.numpy(), ref[1].numpy()) <= BOUND
    assert all(U.scaled_err(g_theta[k].numpy(), ref[2][k].numpy()) <= BOUND for k in g_theta)


def test_sample_rsample_log_prob():
    m, flow, z, G, ctx, tr = _case("cond")
    n = 6
    c = torch.randn(n, 3, generator=torch.Generator().manual_seed(3), dtype=torch.float64)
    a = flow.sample(n, context=c, generator=torch.Generator().manual_seed(5))
    b = flow.sample(n, context=c, generator=torch.Generator().manual_seed(5))
    other = flow.sample(n, context=c, generator=torch.Generator().manual_seed(6))
    assert a.shape == (n, D) and a.dtype == torch.float64 and torch.equal(a, b) and not torch.equal(a, other)
    assert not a.requires_grad and a.grad_fn is None
    z_drawn = torch.randn(n, D, generator=torch.Generator().manual_seed(5), dtype=torch.float64)
    with torch.no_grad():
        assert torch.equal(a, flow.invert(z_drawn, context=c, method="newton"))
        assert float((flow(a, context=c) - z_drawn).abs().max()) < 1e-5
    assert torch.equal(flow.sample(n, context=c, generator=torch.Generator().manual_seed(5), method="jacobi"),
                       flow.invert(z_drawn, context=c, method="jacobi"))
    # rsample: the same draw, with a graph to the parameters and the context
    cc = c.clone().requires_grad_()
    r, info = flow.rsample(n, context=cc, generator=torch.Generator().manual_seed(5), return_info=True)
    assert torch.equal(r.detach(), a) and r.requires_grad
    grads = torch.autograd.grad(r.square().sum(), [cc] + list(flow.parameters()))
    assert all(torch.isfinite(g).all() for g in grads) and float(grads[0].abs().max()) > 0
    assert len(info["adjoint"]) == 2 and all(rec["sweeps"] <= D for rec in info["adjoint"])
    # log_prob is compute_ll's first output
    ll, _ = flow.compute_ll(a, context=c)
    assert torch.equal(flow.log_prob(a, context=c), ll) and ll.shape == (n,)


def test_refusals():
    m, blk, z, G, ctx, tr = _case("block")
    for module in (blk, m):
        with pytest.raises(ValueError, match="bracket"):
            module.inverse(z, method="bracket")
        with pytest.raises(ValueError, match="max_adj_sweeps"):
            module.inverse(z, max_adj_sweeps=-1)
        with pytest.raises(ValueError, match="adj_tol"):
            module.inverse(z, adj_tol=-1.)
    with pytest.raises(ValueError, match="bracket"):
        m.rsample(3, method="bracket")

    class Wrapper(torch.nn.Module):
        def forward(self, zz):
            return m.inverse(zz)
    with pytest.raises(RuntimeError, match="torch.jit.trace"):
        torch.jit.trace(Wrapper(), (z,))


def test_update_in_torch_ops_and_its_flag_word():
    """The fallback of ``integral.flow_adjoint_update`` (host tensors, float64): the formula, in place or not, and the flag rules."""
    g = torch.Generator().manual_seed(0)
    gx, lj, lam = (torch.randn(7, 5, generator=g, dtype=torch.float64) for _ in range(3))
    r = gx - 1e-7 * torch.rand(7, 5, generator=g, dtype=torch.float64)

    def run(r, tol, out=None, lam=lam):
        flags = torch.zeros(1, dtype=torch.int32)
        return integral.flow_adjoint_update(gx, r, lj, lam, tol, flags, out=out), int(flags)
    want = lam + (gx - r) * torch.exp(-lj)
    out, word = run(r, 1e-6)
    assert torch.equal(out, want) and word == 0 and out is not lam
    buf = lam.clone()
    out, word = run(r, 1e-6, out=buf, lam=buf)
    assert out is buf and torch.equal(buf, want)
    assert run(r, 0.)[1] == 1 and run(gx.clone(), 0.)[1] == 0
    r_over = r.clone()
    r_over[3, 2] -= 1e-5 * max(1., abs(float(gx[3, 2])))
    assert run(r_over, 1e-6)[1] == 1
    r_nan = r.clone()
    r_nan[6, 4] = float("nan")
    out, word = run(r_nan, 1e-6)
    assert word == 2 and torch.isnan(out[6, 4]) and torch.equal(out[:6], want[:6])
    r_nan[0, 0] = float("inf")
    assert run(r_nan, 0.)[1] == 3, "the finite entries still report under tol = 0"


def test_entry_point_validates_without_a_gpu():
    lib = _lib.lib()
    p = ctypes.c_void_p(0x1000)

    def call(B=4, d=3, tol=1e-6, g=p, r=p, lj=p, lam=p, out=p, flags=p):
        return lib.umnn_flow_adjoint_update(g, r, lj, lam, B, d, tol, out, flags, None)
    assert call(B=0) == 0                                 # an empty batch is a no-op and touches no device
    assert call(B=-1) == _lib.EINVAL and call(d=0) == _lib.EINVAL and call(tol=-1.) == _lib.EINVAL and call(tol=float("nan")) == _lib.EINVAL
    for name in ("g", "r", "lj", "lam", "out", "flags"):
        assert call(**{name: None}) == _lib.EINVAL, name
    assert b"adjoint" in lib.umnn_last_error()


def test_compiled_callers_get_an_eager_call():
    """Like ``invert``: under torch.compile the solve, its autograd node and the sweeps run eagerly -- the same gradients bit for bit."""
    m, flow, z, G, ctx, tr = _case("flow2")
    params = list(flow.parameters())

    def loss(zz):
        return flow.inverse(zz).square().sum()
    z1, z2 = z.clone().requires_grad_(), z.clone().requires_grad_()
    ref = torch.autograd.grad(loss(z1), [z1] + params)
    out = torch.autograd.grad(torch.compile(loss, backend="eager")(z2), [z2] + params)
    assert all(torch.equal(a, b) for a, b in zip(ref, out))
