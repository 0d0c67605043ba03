"""The g_fx cotangent of the multi-output backward on the device: umnn_cc_backward_multi_fx itself on every family and pass list, the
flag cases, the exact (bit) properties, the large launch; then ``IntegralWithDerivative`` and ``MonotonicNN.forward_with_derivative``
on the GPU, eager and recorded.

Entry-level calls are made in the manner of tests/test_gpu_multi_coverage.py (whose device inputs and output / workspace guards are
reused): outputs pre-filled with NaN with NaN guards behind them, a workspace of exactly umnn_cc_backward_multi_workspace_bytes filled
with 0xFF with a byte pattern behind it.  Truth and bound: tests/_multi_derivative_cases.py -- each output within M x E32 of the
float64 truth, never above 1e-5.  Every case prints its figures as multiples of E32 (profiles/multi_derivative/README.md)."""
import copy
import ctypes
import warnings

import numpy as np
import pytest
import torch

import umnn_amd
from tests import _multi_coverage_cases as C
from tests import _multi_derivative_cases as D
from tests import _multi_output_cases as M
from tests import _util as U
from tests import test_gpu_multi_coverage as G
from umnn_amd import _lib, integral as I
from umnn_amd._common import _ptr, _stream
from umnn_amd.quadrature import device_tables

pytestmark = pytest.mark.gpu
TOL = M.TOL
ALL = (1, 1, 1, 1)
PRECISIONS = [("f16x3", "bf16x3"), ("fp32", "fp32"), ("bf16x3", "bf16x3"), ("bf16x6", "fp32")]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


@pytest.fixture(autouse=True)
def _restore():
    old = umnn_amd.get_forward_precision(), umnn_amd.get_backward_precision()
    yield
    umnn_amd.set_forward_precision(old[0])
    umnn_amd.set_backward_precision(old[1])


_COT = {}


def _cotangents(c, t, dev):
    """(g_fx, zeros like g) of a case on the device, float32; once per case"""
    key = C._input_key(c)
    if key not in _COT:
        _COT[key] = (D.gfx_of(c).float().to(dev).contiguous(), torch.zeros_like(t.g))
    return _COT[key]


def _backward_fx(c, t, dev, need=ALL, lo=0, hi=None, zero_g=False, gfx=True):
    """umnn_cc_backward_multi_fx on sample rows lo..hi -> ([d_x0, d_x, d_h, d_theta], None where not asked for; name of the last pass;
    launches).  zero_g: g = 0; gfx False: a null g_fx."""
    lib = _lib.lib()
    hi = c["B"] if hi is None else hi
    x0, x, h, g = G._rows(t, lo, hi)
    gf, zeros = _cotangents(c, t, dev)
    g = zeros[lo:hi] if zero_g else g
    gf = gf[lo:hi] if gfx else None
    B, d, E = x.shape[0], c["d"], c["E"]
    shapes = [(B, d), (B, d), (B, E * d), (C.n_params(c),)]
    outs = [G._Out(sh, dev) if k and int(np.prod(sh)) else None for k, sh in zip(need, shapes)]
    w, s = device_tables(c["n"], dev)
    pattern = (torch.arange(G.GUARD_BYTES, device=dev) * 37 + 11).to(torch.uint8)
    with torch.cuda.device(dev):
        nbytes = int(lib.umnn_cc_backward_multi_workspace_bytes(ctypes.byref(t.desc), B, d, E))
        assert nbytes > 0, lib.umnn_last_error()
        ws = torch.empty(nbytes + G.GUARD_BYTES, device=dev, dtype=torch.uint8)
        ws[:nbytes] = 0xFF
        ws[nbytes:] = pattern
        before = lib.umnn_launch_count()
        rc = lib.umnn_cc_backward_multi_fx(ctypes.byref(t.desc), _ptr(x0), _ptr(x), G._hptr(t, h), _ptr(g), _ptr(gf), _ptr(w), _ptr(s), c["n"], B, d, E,
                                           int(c["inv_f"]), *(None if o is None else _ptr(o.t) for o in outs), ctypes.c_void_p(ws.data_ptr()), nbytes,
                                           _stream(dev))
        _lib.check(rc, "umnn_cc_backward_multi_fx")
        torch.cuda.synchronize()
        launches = lib.umnn_launch_count() - before
    assert torch.equal(ws[nbytes:], pattern), "the call wrote behind umnn_cc_backward_multi_workspace_bytes()"
    name = lib.umnn_last_kernel_name_of(_lib.PROF_BACKWARD).decode()
    return [None if o is None else o.check(nm) for nm, o in zip(C.GRADS, outs)], name, launches


def _against_truth(c, got, T, tag):
    err, worst = D.errors(got, T.t), {}
    for name, e in err.items():
        es, Es = (e, T.E32[name]) if isinstance(e, list) else ([e], [T.E32[name]])
        worst[name] = max(a / b for a, b in zip(es, Es))
    print(f"MULTIDERIV|{c['fam'][0]},{c['fam'][1]}|{c['id']}|{tag}|" + "|".join(f"{k} {v:.2f}" for k, v in worst.items())
          + "|E32 " + " ".join(f"{k} {(max(v) if isinstance(v, list) else v):.2e}" for k, v in T.E32.items() if k in err))
    for name, e in err.items():
        es, Es = (e, T.E32[name]) if isinstance(e, list) else ([e], [T.E32[name]])
        for j, (a, b) in enumerate(zip(es, Es)):
            assert a <= D.bound(b, name), (c["id"], tag, name, j, a, D.bound(b, name))


_IDS = [f"{c['fam'][0]}x{c['fam'][1]}-{c['id']}" for c in D.DEVICE_CASES]


# ---- every family, pass list and flag, with (g, g_fx) and with (0, g_fx) ---------------------------------------------------------
@pytest.mark.parametrize("zero_g", [False, True], ids=["g+gfx", "gfx"])
@pytest.mark.parametrize("c", D.DEVICE_CASES, ids=_IDS)
def test_case(c, zero_g, dev):
    t = G._on_device(c, dev)
    bwd, name, launches = _backward_fx(c, t, dev, zero_g=zero_g)
    assert name == D.fx_name(c["last"]) and launches == c["passes"], (name, launches)
    again, _, _ = _backward_fx(c, t, dev, zero_g=zero_g)
    for nm, a, b in zip(C.GRADS, bwd, again):
        assert G._equal(a, b), f"{nm}: a second call is not bit-equal"
    # without d_theta: the family's first pass alone (no extra launch: d f / d x comes out of that pass), the bits of the full call
    alone, name, launches = _backward_fx(c, t, dev, (1, 1, 1, 0), zero_g=zero_g)
    assert name == D.fx_name(c["first"]) and launches == 1, (name, launches)
    for nm, a, b in zip(C.GRADS[:3], bwd, alone):
        assert G._equal(a, b), f"{nm}: differs when d_theta is not asked for"
    _against_truth(c, G._as_rows(c, t, None, bwd), D.truth(c, zero_g), "gfx" if zero_g else "g+gfx")


@pytest.mark.parametrize("fam", list(C.REP_CASES), ids=lambda f: f"{f[0]}x{f[1]}")
def test_null_gfx_is_the_old_entry_and_a_null_dx_changes_nothing_else(fam, dev):
    c = C.REP_CASES[fam]
    t = G._on_device(c, dev)
    old, oname, olaunches = G._backward(c, t, dev)
    new, nname, nlaunches = _backward_fx(c, t, dev, gfx=False)
    assert (nname, nlaunches) == (oname, olaunches) == (c["last"], c["passes"])
    for nm, a, b in zip(C.GRADS, old, new):
        assert G._equal(a, b), f"{nm}: g_fx = NULL through the new entry differs from umnn_cc_backward_multi"
    full, _, _ = _backward_fx(c, t, dev)
    assert not torch.equal(full[1], old[1]) and not torch.equal(full[2], old[2])          # (the cotangent is not ignored)
    nodx, name, launches = _backward_fx(c, t, dev, (1, 0, 1, 1))
    assert nodx[1] is None and (name, launches) == (D.fx_name(c["last"]), c["passes"])
    for nm, a, b in zip(C.GRADS, full, nodx):
        assert b is None or torch.equal(a, b), f"{nm}: differs when d_x is not asked for"


def test_large_launch_equals_its_chunks(dev):
    """Shape A of tests/_multi_coverage_cases.py (2 x 4 x CUs + 3 tiles, d = 1, n = 2) on [20, 31, 9]: persistent waves own a second and a
    third group, so the per-group state of the g_fx walk (its cotangent, d f / d x, the dc sums) is re-made per group.  d_x0, d_x and d_h
    hold the bits of launches of the same rows in chunks of at most 8192 integrals; d_theta meets the bound."""
    cus = torch.cuda.get_device_properties(dev).multi_processor_count
    c = C.large_case(C.large_shapes(cus)[0])
    tiles = (c["B"] * c["d"] + 15) // 16
    assert tiles > 2 * 4 * cus and c["n"] == 2
    t = G._on_device(c, dev)
    bwd, name, launches = _backward_fx(c, t, dev)
    assert name == D.fx_name(c["last"]) and launches == c["passes"]
    for lo, hi in G._chunks(c, cus):
        b1, _, _ = _backward_fx(c, t, dev, (1, 1, 1, 0), lo, hi)
        for nm, a, b in zip(C.GRADS[:3], b1, bwd):
            assert torch.equal(a, b[lo:hi]), (nm, lo)
    _against_truth(c, G._as_rows(c, t, None, bwd), D.truth(c), "g+gfx")


# ---- the operator ---------------------------------------------------------------------------------------------------------------------
def _kname():
    return _lib.lib().umnn_last_kernel_name().decode()


def _bname():
    return _lib.lib().umnn_last_kernel_name_of(_lib.PROF_BACKWARD).decode()


def _gfx_for(case):
    return torch.randn(case.B, case.K, generator=torch.Generator().manual_seed(500 + case.seed))


def _pair_grads(op, net, x, h, g, gfx, nb_steps):
    net.zero_grad()
    xr, hr = x.clone().requires_grad_(), h.clone().requires_grad_()
    F, fx = op.apply(torch.zeros_like(xr), xr, net, I._flatten(net.parameters()), hr, nb_steps)
    ((F * g).sum() + (fx * gfx).sum()).backward()
    torch.cuda.synchronize()
    return F.detach(), fx.detach(), xr.grad, hr.grad, [p.grad.clone() for p in net.parameters()]


def _check_pair(tag, got, T):
    F, fx, dx, dh, dps = (v.cpu().numpy() if torch.is_tensor(v) else [p.cpu().numpy() for p in v] for v in got)
    errs = {"F": U.rel_err(F, T[0]), "fx": U.rel_err(fx, T[1]), "dx": U.rel_err(dx, T[2]), "dh": U.scaled_err(dh, T[3]),
            "dtheta": max(U.scaled_err(a, b) for a, b in zip(dps, T[4]))}
    print(f"{tag}: " + " ".join(f"{k} {v:.2e}" for k, v in errs.items()))
    for k, v in errs.items():
        assert v <= TOL, (tag, k, v)


@pytest.mark.parametrize("i", [0, 1, 2, 3])
def test_operator_matches_float64(dev, i):
    c = M.CASES[i]
    net, x, h, g = M.build(c)
    gfx = _gfx_for(c)
    assert M.case_truth(i).margin >= M.MIN_MARGIN
    netg = copy.deepcopy(net).to(dev)
    for tag, gg in (("g+gfx", g), ("gfx", torch.zeros_like(g))):
        got = _pair_grads(umnn_amd.IntegralWithDerivative, netg, x.to(dev), h.to(dev), gg.to(dev), gfx.to(dev), c.nb_steps)
        assert I.path_taken() == "hip" and "multi" in _kname() and I.backward_path_taken() == "hip" and "FX=1" in _bname()
        _check_pair(f"case {i} {tag}", got, D.operator_truth(net, x, h, gg, gfx, c.nb_steps))
    first = None
    for fwd, bwd in PRECISIONS:                          # exact fp32 kernels whatever is set
        umnn_amd.set_forward_precision(fwd)
        umnn_amd.set_backward_precision(bwd)
        got = _pair_grads(umnn_amd.IntegralWithDerivative, netg, x.to(dev), h.to(dev), g.to(dev), gfx.to(dev), c.nb_steps)
        flat = list(got[:4]) + got[4]
        first = flat if first is None else first
        assert all(torch.equal(a, b) for a, b in zip(flat, first)), (fwd, bwd)


def test_seventeen_outputs_run_on_aten_with_one_notice(dev):
    c = M.CASES[4]
    net, x, h, g = M.build(c)
    gfx = _gfx_for(c)
    from umnn_amd import nets
    nets._noticed.discard("wide")
    netg = copy.deepcopy(net).to(dev)
    with warnings.catch_warnings(record=True) as rec:
        warnings.simplefilter("always")
        got = _pair_grads(umnn_amd.IntegralWithDerivative, netg, x.to(dev), h.to(dev), g.to(dev), gfx.to(dev), c.nb_steps)
        assert I.path_taken() == "aten" and I.backward_path_taken() == "aten"
        got = _pair_grads(umnn_amd.IntegralWithDerivative, netg, x.to(dev), h.to(dev), g.to(dev), gfx.to(dev), c.nb_steps)
    assert len([w for w in rec if "n_out = 17" in str(w.message)]) == 1
    assert got[0].shape == (c.B, 17) and got[1].shape == (c.B, 17)
    _check_pair("case 4", got, D.operator_truth(net, x, h, g, gfx, c.nb_steps))


@pytest.mark.parametrize("fwd,bwd", [(None, None), ("fp32", "fp32")], ids=["default", "fp32"])
def test_single_output_is_integral_with_jacobian(dev, fwd, bwd):
    if fwd is not None:
        umnn_amd.set_forward_precision(fwd)
        umnn_amd.set_backward_precision(bwd)
    torch.manual_seed(4)
    net = M.IntegrandNN([3, 50, 50, 50, 1], "LeakyReLU").to(dev)
    gen = torch.Generator().manual_seed(104)
    x, h = (torch.randn(37, 1, generator=gen) * 2).to(dev), torch.randn(37, 2, generator=gen).to(dev)
    g, gfx = torch.randn(37, 1, generator=gen).to(dev), torch.randn(37, 1, generator=gen).to(dev)
    a = _pair_grads(I.IntegralWithJacobian, net, x, h, g, gfx, 20)
    ka, ba = _kname(), _bname()
    b = _pair_grads(umnn_amd.IntegralWithDerivative, net, x, h, g, gfx, 20)
    assert (_kname(), _bname()) == (ka, ba) and "multi" not in ka and I.backward_path_taken() == "hip"
    for u, v in zip(list(a[:4]) + a[4], list(b[:4]) + b[4]):
        assert torch.equal(u, v)


def test_the_forward_op_is_differentiable_in_f_x(dev):
    """``umnn::cc_forward_multi`` called as an op: a loss on f_x (alone, or with F) differentiates through ``umnn::cc_backward_multi_fx``
    and gives the operator's bits; a loss on F alone runs the kernels without g_fx, as before."""
    c = M.CASES[1]
    net, x, h, g = M.build(c)
    gfx = _gfx_for(c).to(dev)
    netg = copy.deepcopy(net).to(dev)
    xg, hg, gg = x.to(dev), h.to(dev), g.to(dev)
    lins = [m for m in netg.net if isinstance(m, torch.nn.Linear)]
    W, b = [l.weight for l in lins], [l.bias for l in lins]

    def run(gF, gf):
        netg.zero_grad()
        xr, hr = xg.clone().requires_grad_(), hg.clone().requires_grad_()
        F, fx = torch.ops.umnn.cc_forward_multi(None, xr, hr, W, b, _lib.ACT_LEAKY_RELU, _lib.OUT_ELU_PLUS_ONE, c.nb_steps, False)
        assert fx.requires_grad
        loss = (0 if gF is None else (F * gF).sum()) + (0 if gf is None else (fx * gf).sum())
        loss.backward()
        return [xr.grad, hr.grad] + [p.grad.clone() for p in netg.parameters()], _bname()

    for gF, gf in ((gg, gfx), (None, gfx)):
        ref = _pair_grads(umnn_amd.IntegralWithDerivative, netg, xg, hg, torch.zeros_like(gg) if gF is None else gF, gf, c.nb_steps)
        got, name = run(gF, gf)
        assert "FX=1" in name
        for u, v in zip(got, list(ref[2:4]) + ref[4]):
            assert torch.equal(u, v)
    got, name = run(gg, None)
    assert "FX" not in name
    xr, hr = xg.clone().requires_grad_(), hg.clone().requires_grad_()
    netg.zero_grad()
    F = I.ParallelNeuralIntegral.apply(torch.zeros_like(xr), xr, netg, I._flatten(netg.parameters()), hr, c.nb_steps)
    (F * gg).sum().backward()
    for u, v in zip(got, [xr.grad, hr.grad] + [p.grad for p in netg.parameters()]):
        assert torch.equal(u, v)


# ---- MonotonicNN ----------------------------------------------------------------------------------------------------------------------
def _mono(dev, nb_steps=20, B=64, K=4):
    torch.manual_seed(3)
    m = umnn_amd.MonotonicNN(3, [100, 100, 100], nb_steps=nb_steps, n_out=K)
    gen = torch.Generator().manual_seed(11)
    x = torch.randn(B, 1, generator=gen) * 2
    h = torch.randn(B, 2, generator=gen)
    delta = torch.nn.functional.one_hot(torch.randint(0, K, (B,), generator=gen), K).float()
    return m, x, h, delta


def _risks_loss(y, log_dy, delta):
    """competing risks: -mean_b sum_k [delta_k log h_k(t) - H_k(t)], H_k = y_k the cumulative hazard, h_k = dy_k/dt the hazard"""
    return -(delta * log_dy - y).sum(1).mean()


def test_monotonic_pair_and_adam_step_match_float64(dev):
    m, x, h, delta = _mono(dev)
    m64 = copy.deepcopy(m).double()
    mg = copy.deepcopy(m).to(dev)
    xg, hg, dg = x.to(dev), h.to(dev), delta.to(dev)
    with torch.no_grad():
        y0 = mg(xg, hg)
        launches = _lib.lib().umnn_launch_count()
        y1, dy = mg.forward_with_derivative(xg, hg)
        assert _lib.lib().umnn_launch_count() == launches + 1 and "multi" in _kname()           # one quadrature launch
        assert torch.equal(y1, y0) and bool((dy > 0).all())
    opt64 = torch.optim.Adam(m64.parameters(), lr=1e-3)
    optg = torch.optim.Adam(mg.parameters(), lr=1e-3)
    loss64 = _risks_loss(*D.mono64(m64, x.double(), h.double(), M.quadrature64), delta.double())
    loss64.backward()
    opt64.step()
    y, ldy = mg.forward_with_derivative(xg, hg, log=True)
    assert torch.equal(y, y0) and I.path_taken() == "hip"
    loss = _risks_loss(y, ldy, dg)
    loss.backward()
    optg.step()
    assert I.backward_path_taken() == "hip" and "FX=1" in _bname()
    e = abs(loss.item() - loss64.item()) / max(abs(loss64.item()), 1.0)
    print(f"loss {loss.item():.6f} vs {loss64.item():.6f}: {e:.2e}")
    assert e <= TOL
    for (name, p), p64 in zip(mg.named_parameters(), m64.parameters()):
        e = U.scaled_err(p.detach().cpu().numpy(), p64.detach().numpy())
        print(f"{name}: {e:.2e}")
        assert e <= TOL, name


def _loss_and_grads(mg, xg, hg, dg, fn):
    mg.zero_grad()
    xr, hr = xg.clone().requires_grad_(), hg.clone().requires_grad_()
    loss = fn(xr, hr, dg)
    loss.backward()
    return [loss.detach(), xr.grad, hr.grad] + [p.grad.clone() for p in mg.parameters()]


def test_compile_fullgraph_is_bit_identical(dev):
    import torch._dynamo
    m, x, h, delta = _mono(dev, nb_steps=10, B=33)
    mg = copy.deepcopy(m).to(dev)
    xg, hg, dg = x.to(dev), h.to(dev), delta.to(dev)

    def fn(xx, hh, dd):
        return _risks_loss(*mg.forward_with_derivative(xx, hh, log=True), dd)

    eager = _loss_and_grads(mg, xg, hg, dg, fn)
    torch._dynamo.reset()
    compiled = _loss_and_grads(mg, xg, hg, dg, torch.compile(fn, fullgraph=True, backend="aot_eager"))
    torch._dynamo.reset()
    assert "multi" in _kname() and I.backward_path_taken() == "hip" and "FX=1" in _bname()
    for a, b in zip(eager, compiled):
        assert a.shape == b.shape and torch.equal(a, b)


class _Pair(torch.nn.Module):
    def __init__(self, m):
        super().__init__()
        self.m = m

    def forward(self, x, h):
        return self.m.forward_with_derivative(x, h, log=True)


def test_export_keeps_the_multi_op(dev):
    m, x, h, _ = _mono(dev, nb_steps=10, B=33)
    mg = _Pair(copy.deepcopy(m).to(dev)).eval()
    xg, hg = x.to(dev), h.to(dev)
    ep = torch.export.export(mg, (xg, hg))
    assert "umnn.cc_forward_multi" in str(ep.graph)
    with torch.no_grad():
        for a, b in zip(ep.module()(xg, hg), mg(xg, hg)):
            assert torch.equal(a, b)
