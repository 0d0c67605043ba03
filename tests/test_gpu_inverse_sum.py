"""The in-kernel Newton solve of a weighted sum of the K monotone outputs (umnn_cc_solve_multi, csrc/cc_multi.hip) on the GPU: every
kernel family, the precision switches, the host-driven loop it replaces, the K = 17 route, flags and non-finite rows inside one tile,
batch shapes, strides, the implicit gradients through the multi-output backward, and graph mode.

Cases, float64 truth and bounds: tests/_inverse_sum_cases.py (values: |x^ - x*| D(x*) <= (1e-5 + tol) max(1, |t|) per row; F, f_x:
1e-5 ``rel_err``; gradients: 1e-5 ``scaled_err``)."""
import copy
import warnings

import numpy as np
import pytest
import torch

import umnn_amd
from tests import _inverse_sum_cases as S
from tests import _inverse_truth as IT
from tests import _multi_output_cases as M
from tests import _util as U
from umnn_amd import _lib, integral as I
from umnn_amd.nets import mlp_spec

pytestmark = pytest.mark.gpu
PRECISIONS = ["f16x3", "fp32", "bf16x3", "bf16x6"]
FLAGS = ~_lib.SOLVE_EVALS_MASK


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


@pytest.fixture(autouse=True)
def _restore():
    old = umnn_amd.get_forward_precision(), umnn_amd.get_backward_precision(), umnn_amd.get_made_fast_path()
    yield
    umnn_amd.set_forward_precision(old[0])
    umnn_amd.set_backward_precision(old[1])
    umnn_amd.set_made_fast_path(old[2])


def _kname():
    return _lib.lib().umnn_last_kernel_name().decode()


def _launches():
    return _lib.lib().umnn_launch_count()


def _on(dev, net, *tensors):
    return (copy.deepcopy(net).to(dev),) + tuple(t.to(dev) for t in tensors)


def _solve(net, t, coef, h, n, info=True, **kw):
    return umnn_amd.InverseIntegralSum.apply(t, coef, net, I._flatten(net.parameters()), h, n, kw.get("x_range", (S.LO, S.HI)),
                                             kw.get("tol", S.SOLVE_TOL), kw.get("max_iter", S.MAX_ITER), info)


def _raw(net, t, coef, h, n, **kw):
    """(x, F, f_x, status) of one umnn_cc_solve_multi launch."""
    out = I.hip_solve_multi(mlp_spec(net), h.contiguous(), t.contiguous(), coef.contiguous(), n, kw.get("lo", S.LO), kw.get("hi", S.HI),
                            kw.get("tol", S.SOLVE_TOL), kw.get("max_iter", S.MAX_ITER))
    assert out is not None
    return out


def _host_loop(net, t, coef, h, n):
    """The host-driven loop the kernel replaces: ``newton_solve`` over ``hip_forward_multi``, one launch per iteration."""
    return I.newton_solve_sum(I.quadrature_eval(mlp_spec(net), None, h, n, True), t, coef, S.LO, S.HI, S.SOLVE_TOL, S.MAX_ITER)


def _same(a, b):
    return all(torch.equal(u, v) for u, v in zip(a, b))


# ------------------------------------------------------------------------------------------------------------ every family
@pytest.mark.parametrize("i", S.KERNEL_CASES)
def test_every_family_matches_float64(dev, i):
    c, d = S.CASES[i], S.value_data(i)
    assert not d.clamped.any() and not d.capped.any()
    netg, tg, cg, hg = _on(dev, d.net, d.t, d.coef, d.h)
    before = _launches()
    with torch.no_grad():
        x, f, status = _solve(netg, tg, cg, hg, c.nb_steps)
    assert _launches() - before == 1
    assert I.path_taken() == "hip" and _kname() == S.kernel_name(i)
    share, ok = S.value_bound(x.cpu().numpy(), d)
    st = status.cpu().numpy()
    gap = int(np.max(np.abs((st & _lib.SOLVE_EVALS_MASK) - d.evals)))
    xr, F, fr, sr = _raw(netg, tg, cg, hg, c.nb_steps)
    F64, f64 = S.parts64(M._double(d.net), x.cpu().numpy(), d.h.numpy(), c.nb_steps)          # float64 at the returned x
    eF, ef = U.rel_err(F.cpu().numpy(), F64), U.rel_err(f.cpu().numpy(), f64)
    print(f"case {i}: {_kname()}  worst row at {share:.3f} of the bound, evaluations within {gap} of newton64, F rel_err {eF:.2e}, "
          f"f_x rel_err {ef:.2e}")
    assert x.shape == (c.B, 1) and f.shape == (c.B, c.K) and status.shape == (c.B, 1) and status.dtype == torch.int32
    assert ok.all() and gap <= 1 and not (st & FLAGS).any()
    assert eF <= 1e-5 and ef <= 1e-5
    assert torch.equal(xr, x) and torch.equal(fr, f) and torch.equal(sr, status)


def test_bits_do_not_depend_on_precision_settings_or_run(dev):
    c, d = S.CASES[1], S.value_data(1)
    netg, tg, cg, hg = _on(dev, d.net, d.t, d.coef, d.h)
    with torch.no_grad():
        want = _solve(netg, tg, cg, hg, c.nb_steps)
        assert _same(_solve(netg, tg, cg, hg, c.nb_steps), want)
        for name in PRECISIONS:
            umnn_amd.set_precision(name)
            assert _same(_solve(netg, tg, cg, hg, c.nb_steps), want), name
            assert _kname() == S.kernel_name(1)


# ------------------------------------------------------------------------------------------------------------ host loop, K = 17
@pytest.mark.parametrize("i", [1, 2, 5])
def test_agrees_with_the_host_driven_loop(dev, i):
    c, d = S.CASES[i], S.value_data(i)
    netg, tg, cg, hg = _on(dev, d.net, d.t, d.coef, d.h)
    with torch.no_grad():
        x, _, _, status = _raw(netg, tg, cg, hg, c.nb_steps)
        before = _launches()
        xh, Fh, fh, sh = _host_loop(netg, tg, cg, hg, c.nb_steps)
        host_launches = _launches() - before
    err = np.abs(x.cpu().numpy().astype(np.float64) - xh.cpu().numpy()) * d.D
    lim = (S.TOL_X + S.SOLVE_TOL) * np.maximum(1., np.abs(d.t.double().numpy()))
    gap = int((status & _lib.SOLVE_EVALS_MASK).sub(sh & _lib.SOLVE_EVALS_MASK).abs().max())
    print(f"case {i}: kernel vs host loop at {np.max(err / lim):.3f} of the bound, evaluations within {gap}; host loop {host_launches} launches")
    assert (err <= lim).all() and gap <= 1 and host_launches >= 3
    assert S.value_bound(xh.cpu().numpy(), d)[1].all()


def test_seventeen_outputs_take_the_host_driven_route(dev):
    from umnn_amd import nets
    c, d = S.CASES[4], S.value_data(4)
    nets._noticed.discard("wide")
    netg, tg, cg, hg = _on(dev, d.net, d.t, d.coef, d.h)
    with warnings.catch_warnings(record=True) as rec:
        warnings.simplefilter("always")
        with torch.no_grad():
            x, f, status = _solve(netg, tg, cg, hg, c.nb_steps)
            _solve(netg, tg, cg, hg, c.nb_steps)
    assert len([w for w in rec if "n_out = 17" in str(w.message)]) == 1
    assert I.path_taken() == "aten" and x.is_cuda and f.shape == (c.B, 17)
    share, ok = S.value_bound(x.cpu().numpy(), d)
    print(f"case 4: worst row at {share:.3f} of the bound")
    assert ok.all() and not (status.cpu().numpy() & FLAGS).any()


# ------------------------------------------------------------------------------------------------------------ one tile, four kinds of row
def _mixed_tile():
    """Sixteen rows of case 1's net on [-20, 20] at max_iter = 3: rows 0..10 converge (targets of x = +-1e-4 (row + 1): two
    evaluations in float64), rows 11, 12 lie below G(lo), rows 13, 14 above G(hi), row 15 (target of x = 10) needs five."""
    c, d = S.CASES[1], S.value_data(1)
    lo, hi = -20., 20.
    h, coef = d.h[:16].clone(), d.coef[:16].clone()
    h[15], coef[15] = d.h[1], d.coef[1]
    G = S.sum_map(M._double(d.net), h.numpy(), coef.numpy(), c.nb_steps)
    xs = np.array([[(-1) ** r * 1e-4 * (r + 1)] for r in range(16)])
    xs[15] = 10.
    t = G(xs)[0]
    G_lo, G_hi = G(np.full((16, 1), lo))[0], G(np.full((16, 1), hi))[0]
    t[11:13] = G_lo[11:13] - 100. * np.abs(G_lo[11:13])
    t[13:15] = G_hi[13:15] + 100. * np.abs(G_hi[13:15])
    t = torch.as_tensor(t).float()
    _, evals, clamped, _ = IT.newton64(G, t.double().numpy(), lo, hi, S.SOLVE_TOL, S.MAX_ITER)
    evals, clamped = evals.reshape(-1), clamped.reshape(-1)
    # what the layout rests on, from the float64 iteration alone (one evaluation of room on either side of max_iter = 3)
    assert (evals[:11] <= 2).all() and not clamped[:11].any() and clamped[11:15].all() and (evals[11:15] <= 2).all() and evals[15] >= 5
    return c, d, t, coef, h, lo, hi, xs


def test_mixed_tile_every_row_carries_its_own_flag(dev):
    c, d, t, coef, h, lo, hi, xs = _mixed_tile()
    netg, tg, cg, hg = _on(dev, d.net, t, coef, h)
    with torch.no_grad():
        x, F, f, status = _raw(netg, tg, cg, hg, c.nb_steps, lo=lo, hi=hi, max_iter=3)
        alone = _raw(netg, tg[:11], cg[:11], hg[:11], c.nb_steps, lo=lo, hi=hi, max_iter=3)
    fl = (status.cpu().numpy() & FLAGS).reshape(-1)
    ev = (status.cpu().numpy() & _lib.SOLVE_EVALS_MASK).reshape(-1)
    print(f"mixed tile: evaluations {ev}, flags {fl >> 16}")
    assert not fl[:11].any() and (fl[11:15] == _lib.SOLVE_CLAMPED).all() and fl[15] == _lib.SOLVE_CAPPED and ev[15] == 3
    xc = x.cpu().numpy().reshape(-1)
    assert (xc[11:13] == lo).all() and (xc[13:15] == hi).all()
    assert np.max(np.abs(xc[:11] - xs[:11, 0])) <= 1e-5                   # (D is of order one here; the value bound proper: the family test)
    assert _same((x[:11], F[:11], f[:11], status[:11]), alone)


@pytest.mark.parametrize("what", ["target", "coef", "embedding"])
def test_a_non_finite_row_leaves_its_tile_alone(dev, what):
    c, d = S.CASES[6], S.value_data(6)
    netg, tg, cg, hg = _on(dev, d.net, d.t[:16], d.coef[:16], d.h[:16])
    with torch.no_grad():
        clean = _raw(netg, tg, cg, hg, c.nb_steps)
        tb, cb, hb = tg.clone(), cg.clone(), hg.clone()
        {"target": tb, "coef": cb, "embedding": hb}[what][5, -1] = float("nan")
        x, F, f, status = _raw(netg, tb, cb, hb, c.nb_steps)
    assert torch.isnan(x[5]).all() and int(status[5]) & FLAGS == _lib.SOLVE_NONFINITE
    keep = [r for r in range(16) if r != 5]
    assert _same((x[keep], F[keep], f[keep], status[keep]), tuple(a[keep] for a in clean))
    assert not torch.isnan(clean[0]).any()


# ------------------------------------------------------------------------------------------------------------ shapes and strides
def test_batch_shapes(dev):
    c, d = S.CASES[7], S.value_data(7)
    netg, tg, cg, hg = _on(dev, d.net, d.t, d.coef, d.h)
    with torch.no_grad():
        full = _solve(netg, tg, cg, hg, c.nb_steps)
        for B in (1, 15, 16, 17, 150):
            x, f, status = _solve(netg, tg[:B], cg[:B], hg[:B], c.nb_steps)
            err = np.abs(x.cpu().numpy().astype(np.float64) - d.x_star[:B]) * d.D[:B]
            lim = (S.TOL_X + S.SOLVE_TOL) * np.maximum(1., np.abs(d.t[:B].double().numpy()))
            assert x.shape == (B, 1) and f.shape == (B, c.K) and (err <= lim).all() and not (status.cpu().numpy() & FLAGS).any(), B
            assert _same((x, f, status), tuple(a[:B] for a in full)), B
        xe, fe, se = _solve(netg, tg[:0], cg[:0], hg[:0], c.nb_steps)
    assert xe.shape == (0, 1) and fe.shape == (0, c.K) and se.shape == (0, 1)


def test_non_contiguous_inputs(dev):
    c, d = S.CASES[5], S.value_data(5)
    netg, tg, cg, hg = _on(dev, d.net, d.t, d.coef, d.h)
    wide = lambda a: torch.stack((a, torch.zeros_like(a)), 2).reshape(a.shape[0], -1)[:, ::2]      # noqa: E731  (column stride 2)
    ts, cs, hs = wide(tg), wide(cg), wide(hg)
    assert not cs.is_contiguous() and not hs.is_contiguous() and torch.equal(cs, cg)
    with torch.no_grad():
        assert _same(_solve(netg, ts, cs, hs, c.nb_steps), _solve(netg, tg, cg, hg, c.nb_steps))
        assert _same(_solve(netg, tg.t().contiguous().t(), cg.t().contiguous().t(), hg.t().contiguous().t(), c.nb_steps),
                     _solve(netg, tg, cg, hg, c.nb_steps))


# ------------------------------------------------------------------------------------------------------------ gradients
@pytest.mark.parametrize("i", S.KERNEL_CASES)
def test_gradients_match_float64(dev, i):
    c = S.CASES[i]
    d, g_t, g_coef, d_h, d_params = S.grad_data(i)
    netg, tg, cg, hg, gx = _on(dev, d.net, d.t, d.coef, d.h, d.g_x)
    tg, cg, hg = (a.requires_grad_() for a in (tg, cg, hg))
    x = _solve(netg, tg, cg, hg, c.nb_steps, info=False)
    assert I.path_taken() == "hip" and _kname() == S.kernel_name(i)
    x.backward(gx)
    bname = _lib.lib().umnn_last_kernel_name_of(_lib.PROF_BACKWARD).decode()
    errs = {"t": U.scaled_err(tg.grad.cpu().numpy(), g_t), "coef": U.scaled_err(cg.grad.cpu().numpy(), g_coef),
            "h": U.scaled_err(hg.grad.cpu().numpy(), d_h)}
    for j, (p, ref) in enumerate(zip(netg.parameters(), d_params)):
        errs[f"theta{j}"] = U.scaled_err(p.grad.cpu().numpy(), ref)
    print(f"case {i}: gradient scaled_err max {max(errs.values()):.2e}  backward {bname}")
    assert I.backward_path_taken() == "hip" and bname.startswith("cc_bwd_multi<")
    assert max(errs.values()) <= S.TOL_G, errs


def test_monotonic_inverse_sum_end_to_end(dev):
    torch.manual_seed(3)
    m = umnn_amd.MonotonicNN(3, [100, 100, 100], nb_steps=20, n_out=4)
    gen = torch.Generator().manual_seed(11)
    x, h, w = torch.randn(64, 1, generator=gen) * 2, torch.randn(64, 2, generator=gen), 0.5 + torch.rand(64, 4, generator=gen)
    mg, xg, hg, wg = _on(dev, m, x, h, w)
    with torch.no_grad():
        y = (wg * mg(xg, hg)).sum(1, keepdim=True)
    yg, hg, wg = (a.clone().requires_grad_() for a in (y, hg, wg))
    before = _launches()
    xh = mg.inverse_sum(yg, hg, wg)
    assert _launches() - before == 1 and I.path_taken() == "hip" and _kname() == "cc_solve_multi<T=7,KS=26>"
    xh.sum().backward()
    assert I.backward_path_taken() == "hip"
    with torch.no_grad():
        back = (wg * mg(xh, hg)).sum(1, keepdim=True)
    print(f"MonotonicNN.inverse_sum: round trip rel_err {U.rel_err(back.cpu().numpy(), y.cpu().numpy()):.2e}")
    assert U.rel_err(back.cpu().numpy(), y.cpu().numpy()) <= 1e-5
    for a in [yg, hg, wg] + list(mg.parameters()):
        assert a.grad is not None and torch.isfinite(a.grad).all()
    cpu = copy.deepcopy(m)
    yc, hc, wc = (a.detach().cpu().requires_grad_() for a in (y, hg, wg))
    cpu.inverse_sum(yc, hc, wc).sum().backward()
    for (name, p), q in zip(mg.named_parameters(), cpu.parameters()):
        assert U.scaled_err(p.grad.cpu().numpy(), q.grad.numpy()) <= 1e-4, name
    assert U.scaled_err(wg.grad.cpu().numpy(), wc.grad.numpy()) <= 1e-4 and U.scaled_err(yg.grad.cpu().numpy(), yc.grad.numpy()) <= 1e-4


# ------------------------------------------------------------------------------------------------------------ op and graph mode
def test_opcheck_cc_solve_multi(dev):
    c, d = S.CASES[1], S.value_data(1)
    netg, t, coef, h = _on(dev, d.net, d.t, d.coef + 0.25, d.h)
    W, b, ha, oa = umnn_amd.ops.spec_args(mlp_spec(netg))
    W, b = [w.detach() for w in W], [v.detach() for v in b]
    torch.library.opcheck(torch.ops.umnn.cc_solve_multi.default, (t, coef, h, W, b, ha, oa, c.nb_steps, -50., 50., 1e-6, 64))
    Wg, bg = [w.clone().requires_grad_() for w in W], [v.clone().requires_grad_() for v in b]
    torch.library.opcheck(torch.ops.umnn.cc_solve_multi.default,
                          (t.clone().requires_grad_(), coef.clone().requires_grad_(), h.clone().requires_grad_(), Wg, bg, ha, oa,
                           c.nb_steps, -50., 50., 1e-6, 64))


class _InverseSum(torch.nn.Module):
    def __init__(self, m):
        super().__init__()
        self.m = m

    def forward(self, y, h, w):
        return self.m.inverse_sum(y, h, w)


def _inverse_sum_grads(mod, y, h, w):
    for p in mod.parameters():
        p.grad = None
    yg, hg, wg = (a.clone().requires_grad_() for a in (y, h, w))
    x = mod(yg, hg, wg)
    x.sum().backward()
    return [x.detach(), yg.grad, hg.grad, wg.grad] + [p.grad.clone() for p in mod.parameters()]


def test_inverse_sum_compiles_and_exports(dev):
    import torch._dynamo
    torch._dynamo.reset()
    torch.manual_seed(0)
    m = umnn_amd.MonotonicNN(3, [20, 33, 17], nb_steps=20, n_out=5).to(dev)
    mod = _InverseSum(m)
    gen = torch.Generator().manual_seed(5)
    y, h, w = torch.randn(96, 1, generator=gen).to(dev), torch.randn(96, 2, generator=gen).to(dev), (0.5 + torch.rand(96, 5, generator=gen)).to(dev)
    want = _inverse_sum_grads(mod, y, h, w)
    got = _inverse_sum_grads(torch.compile(mod, backend="aot_eager", fullgraph=True), y, h, w)
    assert _same(got, want)
    assert umnn_amd.path_taken() == "hip" and umnn_amd.backward_path_taken() == "hip"
    batch = torch.export.Dim("batch", min=2, max=4096)
    for p in m.parameters():
        p.requires_grad_(False)
    ep = torch.export.export(mod, (y[:64], h[:64], w[:64]), dynamic_shapes=({0: batch}, {0: batch}, {0: batch}))
    assert "torch.ops.umnn.cc_solve_multi" in ep.graph_module.print_readable(print_output=False)
    with torch.no_grad():
        assert torch.equal(ep.module()(y[:40], h[:40], w[:40]), mod(y[:40], h[:40], w[:40]))
    torch._dynamo.reset()
