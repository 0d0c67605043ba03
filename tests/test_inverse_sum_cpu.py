"""The inverse of a weighted sum of the K monotone outputs on CPU tensors (``newton_solve_sum`` on the ATen quadrature):
``InverseIntegralSum``, ``MonotonicNN.inverse_sum`` and the C ABI's argument checks.  Cases, truth and bounds: tests/_inverse_sum_cases.py.

Measured on the CPU for the eight cases (printed by the tests below):
  * float64 ``newton64`` converges in 2-5 evaluations on cases 0..4 and in 3-5 on the added cases 5..7; no row clamped or capped;
    the float32 and float64 ATen solves use the same number of evaluations as ``newton64`` on every row but one (case 1, float32: 1 off);
  * the float32 ATen Newton solve's worst row uses 0.081 of the value bound on cases 0..4 and 0.095 on cases 5..7 (float64: 0.089);
  * the float32 implicit gradients are within 8.8e-7 ``scaled_err`` of float64 on cases 0..4 and 1.4e-6 on cases 5..7 (case 5, the
    narrowest net: 1.32e-6): the 1e-5 tolerance leaves more than 7x room."""
import copy
import ctypes
import os

import numpy as np
import pytest
import torch

import umnn_amd
from tests import _inverse_sum_cases as S
from tests import _inverse_truth as IT
from tests import _multi_output_cases as M
from tests import _util as U
from umnn_amd import _lib, integral as I

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ALL = list(range(len(S.CASES)))


def _solve(net, t, coef, h, n, info=True, **kw):
    return umnn_amd.InverseIntegralSum.apply(t, coef, net, I._flatten(net.parameters()), h, n, kw.get("x_range", (S.LO, S.HI)),
                                             kw.get("tol", S.SOLVE_TOL), kw.get("max_iter", S.MAX_ITER), info)


def _flags(status):
    return status.numpy() & ~_lib.SOLVE_EVALS_MASK


def _evals(status):
    return status.numpy() & _lib.SOLVE_EVALS_MASK


# ------------------------------------------------------------------------------------------------------------ values
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("i", ALL)
def test_operator_values(i, dtype):
    c, d = S.CASES[i], S.value_data(i)
    assert not d.clamped.any() and not d.capped.any()
    net = copy.deepcopy(d.net).to(dtype)
    with torch.no_grad():
        x, f, status = _solve(net, d.t.to(dtype), d.coef.to(dtype), d.h.to(dtype), c.nb_steps)
    share, ok = S.value_bound(x.numpy(), d)
    gap = int(np.max(np.abs(_evals(status) - d.evals)))
    print(f"case {i} {dtype}: newton64 evaluations {d.evals.min()}..{d.evals.max()}, worst row at {share:.3f} of the bound, "
          f"evaluation counts differ by at most {gap}")
    assert x.shape == (c.B, 1) and x.dtype == dtype and f.shape == (c.B, c.K) and status.shape == (c.B, 1)
    assert I.path_taken() == "aten"
    assert ok.all()
    assert gap <= 1
    assert not _flags(status).any()
    assert U.rel_err(f.numpy(), d.f) <= 1e-5


def _mono(n_out, seed=3, hidden=(20, 33, 17), nb_steps=20, B=29):
    torch.manual_seed(seed)
    m = umnn_amd.MonotonicNN(3, list(hidden), nb_steps=nb_steps, n_out=n_out)
    gen = torch.Generator().manual_seed(40 + seed)
    x = torch.randn(B, 1, generator=gen) * 2
    h = torch.randn(B, 2, generator=gen)
    w = 0.5 + torch.rand(B, n_out, generator=gen)
    g_x = torch.randn(B, 1, generator=gen)
    return m, x, h, w, g_x


def _mono_sum64(m64, x, h, w):
    """(Y, dY/dx) of the weighted sum of a float64 MonotonicNN's outputs by the plain-torch quadrature (differentiable)."""
    out = m64.net(h)
    K = m64.n_out
    F = M.quadrature64(m64.integrand, torch.zeros_like(x), x, h, m64.nb_steps)
    scale = torch.exp(out[:, K:])
    return (w * (scale * F + out[:, :K])).sum(1, keepdim=True), (w * scale * m64.integrand(x, h)).sum(1, keepdim=True)


def _mono_truth(m, x, h, w):
    """-> (m64, y float32 to give to every run, x* float64 numpy, G)."""
    m64 = copy.deepcopy(m).double()

    def G(xx):
        with torch.no_grad():
            Y, D = _mono_sum64(m64, torch.as_tensor(np.asarray(xx, np.float64)), h.double(), w.double())
        return Y.numpy(), D.numpy()
    y = torch.as_tensor(G(x.numpy())[0]).float()
    return m64, y, IT.solve64(G, y.double().numpy(), S.LO, S.HI), G


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["f32", "f64"])
def test_monotonic_inverse_sum_values(dtype):
    m, x, h, w, _ = _mono(5)
    m64, y, x_star, G = _mono_truth(m, x, h, w)
    md = copy.deepcopy(m).to(dtype)
    with torch.no_grad():
        xh, f, status = md.inverse_sum(y.to(dtype), h.to(dtype), w.to(dtype), return_info=True)
        back = (w.to(dtype) * md(xh, h.to(dtype))).sum(1, keepdim=True)
    # the bound in units of the solver's own target t = y - sum_k w_k o_k(h)
    out = m64.net(h.double()).detach()
    t = (y.double() - (w.double() * out[:, :5]).sum(1, keepdim=True)).numpy()
    err = np.abs(xh.numpy().astype(np.float64) - x_star) * G(x_star)[1]
    lim = (S.TOL_X + S.SOLVE_TOL) * np.maximum(1., np.abs(t))
    print(f"MonotonicNN.inverse_sum {dtype}: worst row at {np.max(err / lim):.3f} of the bound; round trip {U.rel_err(back.numpy(), y.numpy()):.2e}")
    assert xh.shape == (29, 1) and f.shape == (29, 5) and (err <= lim).all()
    assert not _flags(status).any()


# ------------------------------------------------------------------------------------------------------------ gradients
@pytest.mark.parametrize("i", ALL)
def test_operator_gradients(i):
    c = S.CASES[i]
    d, g_t, g_coef, d_h, d_params = S.grad_data(i)
    net = copy.deepcopy(d.net)
    t, coef, h = d.t.clone().requires_grad_(), d.coef.clone().requires_grad_(), d.h.clone().requires_grad_()
    x = _solve(net, t, coef, h, c.nb_steps, info=False)
    x.backward(d.g_x)
    errs = {"t": U.scaled_err(t.grad.numpy(), g_t), "coef": U.scaled_err(coef.grad.numpy(), g_coef), "h": U.scaled_err(h.grad.numpy(), d_h)}
    for j, (p, ref) in enumerate(zip(net.parameters(), d_params)):
        errs[f"theta{j}"] = U.scaled_err(p.grad.numpy(), ref)
    print(f"case {i}: gradient scaled_err max {max(errs.values()):.2e}  {({k: f'{v:.1e}' for k, v in errs.items()})}")
    assert I.backward_path_taken() == "aten"
    assert max(errs.values()) <= S.TOL_G, errs


def test_monotonic_inverse_sum_gradients():
    """y, weights, h and every parameter of both networks against float64 autograd through one exact Newton correction at x*:
    x = x* - (Y(x*) - y) / D has the implicit function's first derivatives."""
    m, x, h, w, g_x = _mono(5)
    m64, y, x_star, _ = _mono_truth(m, x, h, w)
    y64, h64, w64 = (a.double().clone().requires_grad_() for a in (y, h, w))
    xs = torch.as_tensor(x_star)
    Y, D = _mono_sum64(m64, xs, h64, w64)
    (xs - (Y - y64) / D.detach()).backward(g_x.double())
    yg, hg, wg = (a.clone().requires_grad_() for a in (y, h, w))
    m.inverse_sum(yg, hg, wg).backward(g_x)
    errs = {"y": U.scaled_err(yg.grad.numpy(), y64.grad.numpy()), "weights": U.scaled_err(wg.grad.numpy(), w64.grad.numpy()),
            "h": U.scaled_err(hg.grad.numpy(), h64.grad.numpy())}
    for (name, p), p64 in zip(m.named_parameters(), m64.parameters()):
        errs[name] = U.scaled_err(p.grad.numpy(), p64.grad.numpy())
    print(f"MonotonicNN.inverse_sum: gradient scaled_err max {max(errs.values()):.2e}")
    assert len(errs) == 3 + len(list(m.parameters())) and max(errs.values()) <= S.TOL_G, errs


# ------------------------------------------------------------------------------------------------------------ weights
def test_one_hot_weights_agree_with_inverse_of_one_output():
    m, x, h, _, _ = _mono(4)
    with torch.no_grad():
        y_all = m(x, h)
        for k in range(4):
            e = torch.zeros(4)
            e[k] = 1.
            y = y_all[:, [k]]
            xs = m.inverse_sum(y, h, e)
            x1, f1, _ = m.inverse(y, h, output=k, return_info=True)
            out = m.net(h)
            t = (y - out[:, [k]]) * torch.exp(-out[:, [4 + k]])                   # the single-output solve's target: D = f_k
            lim = (S.TOL_X + S.SOLVE_TOL) * t.abs().clamp(min=1.)
            assert ((xs - x1).abs() * f1 <= lim).all()


def test_weight_shapes_and_single_output():
    m, x, h, w, _ = _mono(3)
    with torch.no_grad():
        y = (w[0] * m(x, h)).sum(1, keepdim=True)
        a = m.inverse_sum(y, h, w[0])                                # [K]
        b = m.inverse_sum(y, h, w[0].expand(29, 3).contiguous())     # [B,K]
        assert torch.equal(a, b)
        y1 = m(x, h).sum(1, keepdim=True)
        assert torch.equal(m.inverse_sum(y1, h), m.inverse_sum(y1, h, torch.ones(29, 3)))
        m1, x, h, _, _ = _mono(1)
        y = 1.7 * m1(x, h)
        out = m1.net(h)
        for ws, ys in ((torch.tensor([1.7]), y / 1.7), (None, y)):      # n_out = 1: ``inverse`` of the rescaled target
            x1, f1, _ = m1.inverse(ys, h, return_info=True)
            lim = (S.TOL_X + S.SOLVE_TOL) * ((ys - out[:, [0]]) * torch.exp(-out[:, [1]])).abs().clamp(min=1.)
            assert ((m1.inverse_sum(ys * (1. if ws is None else 1.7), h, ws) - x1).abs() * f1 <= lim).all()


# ------------------------------------------------------------------------------------------------------------ edge rows
def test_edge_rows():
    c, d = S.CASES[1], S.value_data(1)
    lo, hi = -20., 20.
    G_lo, G_hi = (d.G(np.full((c.B, 1), v))[0] for v in (lo, hi))
    t = d.t.clone()
    t[0], t[1], t[2] = float(G_lo[0, 0]) - 1., float(G_hi[1, 0]) + 1., float("nan")
    with torch.no_grad():
        x, f, status = _solve(d.net, t, d.coef, d.h, c.nb_steps, x_range=(lo, hi))
        x0, _, status0 = _solve(d.net, d.t, d.coef, d.h, c.nb_steps, x_range=(lo, hi))
    fl = _flags(status).reshape(-1)
    assert x[0] == lo and fl[0] == _lib.SOLVE_CLAMPED and x[1] == hi and fl[1] == _lib.SOLVE_CLAMPED
    assert torch.isnan(x[2]) and fl[2] == _lib.SOLVE_NONFINITE
    assert torch.equal(x[3:], x0[3:]) and torch.equal(status[3:], status0[3:]) and not fl[3:].any()
    with torch.no_grad():          # a row of zero weights follows the clamping rule
        cz = d.coef.clone()
        cz[4] = 0.
        xz, _, sz = _solve(d.net, d.t.abs() + 1., cz, d.h, c.nb_steps, x_range=(lo, hi))
    assert xz[4] == hi and _flags(sz).reshape(-1)[4] == _lib.SOLVE_CLAMPED
    with torch.no_grad():
        x1, _, s1 = _solve(d.net, d.t, d.coef, d.h, c.nb_steps, max_iter=1)
    assert torch.equal(x1, torch.zeros_like(x1)) and (s1 == (1 | _lib.SOLVE_CAPPED)).all()
    with torch.no_grad():
        xe, fe, se = _solve(d.net, d.t[:0], d.coef[:0], d.h[:0], c.nb_steps)
    assert xe.shape == (0, 1) and fe.shape == (0, c.K) and se.shape == (0, 1) and se.dtype == torch.int32


def test_operator_refuses_a_single_curve():
    d = S.value_data(0)
    with pytest.raises(RuntimeError, match="K >= 2"):
        _solve(d.net, d.t, d.coef[:, :1], d.h, 7)


# ------------------------------------------------------------------------------------------------------------ C ABI
def _desc(widths, ptr=0x1000):
    d = _lib.MlpDesc()
    d.n_linear = len(widths) - 1
    for j, w in enumerate(widths):
        d.widths[j] = w
    for l in range(d.n_linear):
        d.W[l], d.b[l] = ptr, ptr
    return d


def test_c_abi_argument_checks_without_gpu():
    lib = _lib.lib()
    p = ctypes.c_void_p(0x1000)

    def call(net, B=4, E=2, n=20, lo=-50., hi=50., tol=1e-6, max_iter=64):
        return lib.umnn_cc_solve_multi(None if net is None else ctypes.byref(net), p, p, p, p, p, n, B, E, lo, hi, tol, max_iter,
                                       p, None, None, None, None)
    ok = _desc([3, 16, 16, 4])
    assert call(None) == _lib.EINVAL
    assert call(_desc([3, 16, 16, 1])) == _lib.EINVAL
    assert call(_desc([3, 16, 16, 17])) == _lib.EINVAL
    assert call(ok, max_iter=0) == _lib.EINVAL and call(ok, max_iter=65536) == _lib.EINVAL
    assert call(ok, lo=1., hi=1.) == _lib.EINVAL and call(ok, lo=2., hi=1.) == _lib.EINVAL
    assert call(ok, n=0) == _lib.EINVAL and call(ok, tol=-1.) == _lib.EINVAL and call(ok, B=-1) == _lib.EINVAL
    assert call(_desc([3] + [80] * 6 + [4])) == _lib.EUNSUPPORTED and b"160 KiB of LDS" in lib.umnn_last_error()
    assert call(ok, B=0) == 0
    assert lib.umnn_cc_solve_multi(ctypes.byref(ok), p, None, p, p, p, 20, 4, 2, -50., 50., 1e-6, 64, p, None, None, None, None) == _lib.EINVAL
    header = open(os.path.join(ROOT, "include", "umnn_cc.h")).read()
    assert "int umnn_cc_solve_multi(const umnn_mlp* net, const float* h, const float* target, const float* coef," in header
    assert "umnn_cc_solve_multi" in _lib.SIGNATURES
