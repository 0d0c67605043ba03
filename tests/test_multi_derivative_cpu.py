"""Differentiable (y, dy/dx) for every n_out, without a GPU: the truth helper of tests/_multi_derivative_cases.py pinned, the
``IntegralWithDerivative`` operator and ``MonotonicNN.forward_with_derivative`` on CPU tensors (the ATen implementation) against
float64, the new C entry's declaration and argument checks, and the new op's registration."""
import copy
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import umnn_amd
from tests import _multi_coverage_cases as C
from tests import _multi_derivative_cases as D
from tests import _multi_output_cases as M
from tests import _util as U
from umnn_amd import _lib, integral as I, ops

TOL = M.TOL
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------------------------------------------------ the truth helper
@pytest.mark.parametrize("fam", list(C.REP_CASES), ids=lambda f: f"{f[0]}x{f[1]}")
def test_truth_with_zero_gfx_is_the_coverage_truth(fam):
    c = C.REP_CASES[fam]
    i = C.inputs(c)
    got = D.case_quadrature_fx(c, i, torch.float64, gfx=torch.zeros_like(D.gfx_of(c)))
    ref = C.truth(c).t
    for name, e in D.errors(got, ref).items():
        assert max(e) <= 1e-12 if isinstance(e, list) else e <= 1e-12, (name, e)
    assert np.abs(got.dxfx).max() == 0.0


@pytest.mark.parametrize("cid", ["p1-20x31x9", "p2-63x52x60-sigmoid", "p2-80x103x70-relu"])
def test_truth_df_dx_agrees_with_a_central_difference(cid):
    """The d f / d x term of the truth -- a derivative of the MLP, not of the quadrature -- against (phi(x + s) - phi(x - s)) / (2 s),
    phi = sum_k f_k(x) g_fx,k per kept row, in float64 with s = 1e-7.  Round-off is about 2^-52 |phi| / s = 2e-9 |phi|, truncation
    s^2 |phi'''| / 6 about 1e-14, and the kept rows have no kink within the step (margin >= 1e-5): the bound is 1e-6 of the largest
    |d phi / d x|; the agreement reached is 8e-9, 8e-9 and 1.3e-8 on the three cases."""
    c = C.BY_ID[cid]
    i = C.inputs(c)
    seq = copy.deepcopy(i.net.net).double()
    x, h = C.rows_of(i.x, i.h, c["d"])
    gfx = D.gfx_of(c).reshape(-1, c["K"])
    step = 1e-7
    with torch.no_grad():
        phi = lambda xv: (seq(torch.cat((xv[:, None], h), 1)) * gfx).sum(1)
        fd = ((phi(x + step) - phi(x - step)) / (2 * step)).numpy()
    got = D.truth(c).t.dxfx
    e = U.rel_err(got, fd)
    print(f"{cid}: d f / d x against a central difference, step {step:g}: {e:.2e}")
    assert e <= 1e-6


def test_inputs_stay_under_the_rejection_cap_and_the_float32_run_is_close():
    """What the bounds rest on: the existing input sets reject at most half of their rows, and the float32 run of the truth's own
    arithmetic is within 1e-5 / 4 of the float64 one on every case the device test uses, with g and with g = 0."""
    worst = 0.0
    for c in D.DEVICE_CASES:
        assert C.inputs(c).reject <= C.REJECT_CAP, c["id"]
        for zero_g in (False, True):
            E = D.truth(c, zero_g).E32
            worst = max(worst, E["dx"], E["dh"], max(E["dtheta"]))
    print(f"largest E32 over the device cases: {worst:.2e}")
    assert worst <= C.OUTER / 4


# ------------------------------------------------------------------------------------------------------------ the operator on CPU tensors
def _net(K, seed=5, act="LeakyReLU"):
    torch.manual_seed(seed)
    return M.IntegrandNN([3, 20, 33, 17, K], act)


@pytest.mark.parametrize("K", [1, 4, 17])
@pytest.mark.parametrize("zero_g", [False, True], ids=["g+gfx", "gfx"])
def test_operator_on_cpu_tensors(K, zero_g):
    net = _net(K)
    gen = torch.Generator().manual_seed(40 + K)
    B, n = 23, 20
    x, h = torch.randn(B, 1, generator=gen) * 2, torch.randn(B, 2, generator=gen)
    g, gfx = torch.randn(B, K, generator=gen), torch.randn(B, K, generator=gen)
    g = torch.zeros_like(g) if zero_g else g
    assert M.margin(net, None, x, h, n) >= M.MIN_MARGIN
    F64, fx64, dx64, dh64, dp64 = D.operator_truth(net, x, h, g, gfx, n)
    xr, hr = x.clone().requires_grad_(), h.clone().requires_grad_()
    F, fx = umnn_amd.IntegralWithDerivative.apply(torch.zeros_like(xr), xr, net, I._flatten(net.parameters()), hr, n)
    assert F.shape == (B, K) and fx.shape == (B, K) and I.path_taken() == "aten"
    ((F * g).sum() + (fx * gfx).sum()).backward()
    assert I.backward_path_taken() == "aten"
    assert U.rel_err(F.detach().numpy(), F64) <= TOL and U.rel_err(fx.detach().numpy(), fx64) <= TOL
    assert xr.grad.shape == (B, 1) and U.rel_err(xr.grad.numpy(), dx64) <= TOL
    assert U.scaled_err(hr.grad.numpy(), dh64) <= TOL
    for p, t in zip(net.parameters(), dp64):
        assert U.scaled_err(p.grad.numpy(), t) <= TOL
    with pytest.raises(RuntimeError):                  # double backward stays out of scope: once_differentiable
        x2 = x.clone().requires_grad_()
        F2, fx2 = umnn_amd.IntegralWithDerivative.apply(torch.zeros_like(x2), x2, net, I._flatten(net.parameters()), h, n)
        (gx,) = torch.autograd.grad(fx2.sum(), x2, create_graph=True)
        gx.sum().backward()


def test_operator_takes_any_callable_and_more_than_one_dimension():
    """Single-output integrands over x [B, d] on ATen: an arbitrary callable, F and f_x [B, d]."""
    f = lambda x, h: torch.exp(-x * x) + h[:, :x.shape[1]] ** 2 + 0.5
    x = torch.linspace(-1, 1, 10, dtype=torch.float64).view(5, 2).clone().requires_grad_()
    h = torch.full((5, 2), 0.3, dtype=torch.float64)
    F, fx = umnn_amd.IntegralWithDerivative.apply(torch.zeros_like(x), x, f, torch.tensor([]), h, 40)
    assert torch.allclose(fx, f(x, h))
    (F.sum() + (fx * fx).sum()).backward()
    xd = x.detach()
    want = f(xd, h) + 2 * f(xd, h) * (-2 * xd * torch.exp(-xd * xd))
    assert torch.allclose(x.grad, want, atol=1e-12)


# ------------------------------------------------------------------------------------------------------------ MonotonicNN
@pytest.mark.parametrize("K", [1, 3])
def test_forward_with_derivative(K):
    torch.manual_seed(7)
    m = umnn_amd.MonotonicNN(3, [20, 33, 17], nb_steps=20, n_out=K)
    gen = torch.Generator().manual_seed(70 + K)
    B = 19
    x, h = torch.randn(B, 1, generator=gen) * 2, torch.randn(B, 2, generator=gen)
    with torch.no_grad():
        y0 = m(x, h)
        y, dy = m.forward_with_derivative(x, h)
        y1, ldy = m.forward_with_derivative(x, h, log=True)
        out = m.net(h)
        s = out[:, [1]] if K == 1 else out[:, K:]
        f = m.integrand(x, h)
    assert y.shape == (B, K) and dy.shape == (B, K)
    assert torch.equal(y, y0) and torch.equal(y1, y0)
    assert bool((dy > 0).all()) and torch.equal(dy, torch.exp(s) * f) and torch.equal(ldy, s + torch.log(f))

    def loss_of(model, xx, hh, fwd):
        yy, ld = fwd(model, xx, hh)
        return -ld.mean() + yy.square().mean()

    xr, hr = x.clone().requires_grad_(), h.clone().requires_grad_()
    loss = loss_of(m, xr, hr, lambda mm, a, b: mm.forward_with_derivative(a, b, log=True))
    loss.backward()
    m64 = copy.deepcopy(m).double()
    m64.zero_grad()
    x64, h64 = x.double().requires_grad_(), h.double().requires_grad_()
    loss64 = loss_of(m64, x64, h64, lambda mm, a, b: D.mono64(mm, a, b, M.quadrature64))
    loss64.backward()
    assert abs(loss.item() - loss64.item()) <= TOL * max(1.0, abs(loss64.item()))
    assert U.rel_err(xr.grad.numpy(), x64.grad.numpy()) <= TOL and U.scaled_err(hr.grad.numpy(), h64.grad.numpy()) <= TOL
    for (name, p), q in zip(m.named_parameters(), m64.parameters()):
        assert p.grad is not None and U.scaled_err(p.grad.numpy(), q.grad.numpy()) <= TOL, name
    # the same loss through the exponentiated second output
    m.zero_grad()
    x2 = x.clone().requires_grad_()
    yy, dd = m.forward_with_derivative(x2, h)
    (-torch.log(dd).mean() + yy.square().mean()).backward()
    assert U.rel_err(x2.grad.numpy(), x64.grad.numpy()) <= TOL
    # what this method replaces keeps raising
    x3 = x.clone().requires_grad_()
    with pytest.raises(RuntimeError):
        (gx,) = torch.autograd.grad(m(x3, h).sum(), x3, create_graph=True)
        gx.sum().backward()


def test_public_names():
    assert umnn_amd.IntegralWithDerivative is I.IntegralWithDerivative and "IntegralWithDerivative" in umnn_amd.__all__
    assert "create_graph" in umnn_amd.MonotonicNN.forward_with_derivative.__doc__


# ------------------------------------------------------------------------------------------------------------ C ABI
def _desc(widths, ptr=0x1000):
    return C.desc(dict(E=widths[0] - 1, hid=list(widths[1:-1]), K=widths[-1], act=_lib.ACT_LEAKY_RELU, out_act=_lib.OUT_ELU_PLUS_ONE), ptr)


def test_abi_entry_is_declared_exported_and_checks_its_arguments():
    name = "umnn_cc_backward_multi_fx"
    header = open(os.path.join(ROOT, "include", "umnn_cc.h")).read()
    assert re.search(r"\bint\s+" + name + r"\s*\(", header)
    assert "There is no g_fx input" not in header
    assert hasattr(ctypes.CDLL(_lib.LIB_PATH), name) and name in _lib.SIGNATURES
    old, new = _lib.SIGNATURES["umnn_cc_backward_multi"], _lib.SIGNATURES[name]
    assert new[0] is ctypes.c_int and len(new[1]) == len(old[1]) + 1 == 20
    lib = _lib.lib()
    p = ctypes.c_void_p(0x1000)

    def both(desc, B=4, dtheta=None):
        """(rc, message) of the old entry and of the new one, with and without a g_fx"""
        out = []
        for gfx in ("old", None, p):
            if gfx == "old":
                rc = lib.umnn_cc_backward_multi(ctypes.byref(desc), None, p, p, p, p, p, 20, B, 1, 2, 0, None, None, None, dtheta, p, 1 << 20, None)
            else:
                rc = lib.umnn_cc_backward_multi_fx(ctypes.byref(desc), None, p, p, p, gfx, p, p, 20, B, 1, 2, 0, None, None, None, dtheta, p, 1 << 20, None)
            out.append((rc, lib.umnn_last_error() if rc else b""))
        return out

    for K in (1, 17):
        res = both(_desc([3, 16, 16, K]))
        assert res[0][0] == _lib.EINVAL and b"output width" in res[0][1] and res[1] == res[0] and res[2] == res[0], K
    res = both(_desc([3, 127, 127, 127, 127, 127, 127, 5]))
    assert res[0][0] == _lib.EUNSUPPORTED and b"LDS" in res[0][1] and res[1] == res[0] and res[2] == res[0]
    assert [r[0] for r in both(_desc([3, 16, 16, 4]), B=0)] == [0, 0, 0]
    four = _desc([3, 16, 16, 4])
    rc = lib.umnn_cc_backward_multi_fx(ctypes.byref(four), None, None, p, p, p, p, p, 20, 4, 1, 2, 0, None, None, None, None, p, 1 << 20, None)
    assert rc == _lib.EINVAL and b"non-null" in lib.umnn_last_error()
    rc = lib.umnn_cc_backward_multi_fx(ctypes.byref(four), None, p, p, p, p, p, p, 0, 4, 1, 2, 0, None, None, None, None, p, 1 << 20, None)
    assert rc == _lib.EINVAL and b"nb_steps" in lib.umnn_last_error()


# ------------------------------------------------------------------------------------------------------------ ops
def test_op_is_registered_with_a_fake():
    from torch._subclasses.fake_tensor import FakeTensorMode
    assert "cc_backward_multi_fx" in ops.OPS and hasattr(torch.ops.umnn, "cc_backward_multi_fx")
    B, E, K, hid = 9, 2, 4, [20, 12]
    widths = [1 + E] + hid + [K]
    n_params = sum(widths[i] * widths[i + 1] + widths[i + 1] for i in range(len(widths) - 1))
    with FakeTensorMode():
        dev = torch.device("cuda")
        x, h = torch.empty(B, 1, device=dev), torch.empty(B, E, device=dev)
        g, gfx = torch.empty(B, K, device=dev), torch.empty(B, K, device=dev)
        W = [torch.empty(widths[i + 1], widths[i], device=dev) for i in range(len(widths) - 1)]
        b = [torch.empty(widths[i + 1], device=dev) for i in range(len(widths) - 1)]
        for mask in C.NEED_MASKS:
            for x0 in (None, torch.empty(B, 1, device=dev)):
                for gf in (gfx, None):
                    out = torch.ops.umnn.cc_backward_multi_fx(x0, x, h, g, gf, W, b, _lib.ACT_RELU, _lib.OUT_ELU_PLUS_ONE, 20, [bool(v) for v in mask], False)
                    want = [(B, 1) if mask[0] and x0 is not None else (0,), (B, 1) if mask[1] else (0,), (B, E) if mask[2] else (0,),
                            (n_params,) if mask[3] else (0,)]
                    assert [tuple(o.shape) for o in out] == want, (mask, x0 is None)
                    assert out[3].dtype == torch.float32
        with pytest.raises(RuntimeError, match="g_fx"):
            torch.ops.umnn.cc_backward_multi_fx(None, x, h, g, torch.empty(B, K + 1, device=dev), W, b, _lib.ACT_RELU, _lib.OUT_ELU_PLUS_ONE, 20, [True] * 4, False)
