"""Whole curves from one quadrature, on the CPU: the cumulative matrix, ``aten_curve`` / ``IntegralCurve``, ``MonotonicNN.forward_curve``
and ``cumulative_incidence`` on the ATen path, and the refusals of the two ops' fakes.  Cases, truth and tolerances:
tests/_curve_cases.py."""
import copy
import warnings

import numpy as np
import pytest
import torch

import umnn_amd
from tests import _curve_cases as C
from tests import _util as U
from umnn_amd import integral as I
from umnn_amd import ops
from umnn_amd.quadrature import _tables_f64, cc_cumulative_matrix, device_cumulative_matrix

NS = [1, 2, 7, 8, 20, 50, 51, 100]


# ---- the table --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", NS)
def test_row_0_is_the_weights_and_row_n_is_zero(n):
    Q = cc_cumulative_matrix(n)
    w, _ = _tables_f64(n)
    assert Q.shape == (n + 1, n + 1) and Q.dtype == np.float64
    assert np.abs(Q[0] - w).max() <= 1e-14
    assert np.all(Q[n] == 0.)
    assert cc_cumulative_matrix(n) is Q                                   # cached like the weights


@pytest.mark.parametrize("n", NS)
def test_integrates_polynomials_below_degree_n_exactly_at_every_node(n):
    # (degree n itself is where the reference's unhalved last coefficient shows: not asked for)
    Q = cc_cumulative_matrix(n)
    _, s = _tables_f64(n)
    for deg in range(n):
        exact = (s ** (deg + 1) - (-1.) ** (deg + 1)) / (deg + 1)            # int_{-1}^{s_i} s^deg
        assert np.abs(Q @ s ** deg - exact).max() <= 1e-12, deg


def test_device_copy_is_fp32_cached_and_reverses_columns():
    Q = cc_cumulative_matrix(7)
    a, b = device_cumulative_matrix(7, "cpu"), device_cumulative_matrix(7, "cpu", ascending=True)
    assert a.dtype == torch.float32 and device_cumulative_matrix(7, "cpu") is a
    assert np.array_equal(a.numpy(), Q.astype(np.float32)) and np.array_equal(b.numpy(), Q[:, ::-1].astype(np.float32))
    assert device_cumulative_matrix(7, "cpu", dtype=torch.float64).dtype == torch.float64


# ---- forward_curve on the CPU -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("i", range(len(C.CASES)))
def test_forward_curve_cpu_matches_float64(i):
    c = C.CASES[i]
    model, x, h = C.build(c)
    T = C.case_truth(i)
    with torch.no_grad(), warnings.catch_warnings():
        warnings.simplefilter("ignore")
        t, y, dy = model.forward_curve(x, h, with_derivative=True)
        assert I.path_taken() == "aten"
        yx = model(x, h)
    n = c.nb_steps
    assert t.shape == (c.B, n + 1) and y.shape == dy.shape == (c.B, n + 1, c.K)
    errs = [U.rel_err(a.numpy(), b) for a, b in ((t, T.t), (y, T.y), (dy, T.dy))]
    print(f"case {i}: float32 ATen vs float64: t {errs[0]:.2e} y {errs[1]:.2e} dy {errs[2]:.2e}; margin {T.margin:.2e}")
    assert T.margin >= C.MIN_MARGIN and max(errs) <= C.TOL
    assert torch.equal(t[:, 0], torch.zeros(c.B)) and torch.equal(t[:, n:], x)
    assert U.rel_err(y[:, n].numpy(), yx.numpy()) <= C.TOL                     # the end point is forward(x, h)
    step = (t[:, 1:] - t[:, :-1]) * torch.sign(x)
    assert bool((step > 0).all())                                              # ascending for x > 0, descending for x < 0
    assert bool((dy > 0).all()) and bool((((y[:, 1:] - y[:, :-1]) * torch.sign(x).unsqueeze(2)) > 0).all())
    t2, y2 = model.forward_curve(x, h)[:2]
    assert len(model.forward_curve(x, h)) == 2 and torch.equal(t2, t)


def test_k17_and_float64_take_the_aten_path():
    model, x, h = C.build(C.CASES[4])
    assert C.CASES[4].K == 17
    with torch.no_grad(), warnings.catch_warnings():
        warnings.simplefilter("ignore")
        I._state.path = None
        t, y = model.forward_curve(x, h)
        assert I.path_taken() == "aten" and y.shape == (33, 21, 17)
        m64, x64, h64 = copy.deepcopy(C.build(C.CASES[0])[0]).double(), *(a.double() for a in C.build(C.CASES[0])[1:])
        I._state.path = None
        t, y, dy = m64.forward_curve(x64, h64, with_derivative=True)
        assert I.path_taken() == "aten" and y.dtype == torch.float64
        T = C.case_truth(0)
        assert U.rel_err(y.numpy(), T.y) <= 1e-12 and U.rel_err(dy.numpy(), T.dy) <= 1e-12 and U.rel_err(t.numpy(), T.t) <= 1e-12


def test_operator_with_nonzero_x0():
    net, x, h, _ = C.M.build(C.X0_CASE)
    x0 = C.x0_of()
    n = C.X0_CASE.nb_steps
    t64, C64, f64 = (a.detach().numpy() for a in C.curve64(copy.deepcopy(net).double(), x0.double(), x.double(), h.double(), n))
    with torch.no_grad(), warnings.catch_warnings():
        warnings.simplefilter("ignore")
        t, Cv, f = umnn_amd.IntegralCurve.apply(x0, x, net, None, h, n)
        F = I.aten_forward(net, x0, x, h, n)
    assert umnn_amd.IntegralCurve is I.IntegralCurve and "IntegralCurve" in umnn_amd.__all__
    assert max(U.rel_err(t.numpy(), t64), U.rel_err(Cv.numpy(), C64), U.rel_err(f.numpy(), f64)) <= C.TOL
    assert torch.equal(t[:, 0], x0[:, 0]) and torch.equal(t[:, n], x[:, 0]) and torch.equal(Cv[:, 0], torch.zeros(C.X0_CASE.B, 5))
    assert U.rel_err(Cv[:, n].numpy(), F.numpy()) <= C.TOL
    with pytest.raises(RuntimeError, match=r"\[B, 1\]"):
        umnn_amd.IntegralCurve.apply(None, torch.zeros(4, 2), net, None, torch.zeros(4, 2), n)


def test_gradcheck_of_aten_curve_in_float64():
    net, x, h, _ = C.M.build(C.M.CASES[0])
    net = copy.deepcopy(net).double()
    x, h = x[:3].double().requires_grad_(), h[:3].double().requires_grad_()
    x0 = (x.detach() * 0.25).requires_grad_()
    params = list(net.parameters())

    def fn(x0, x, h, *ps):
        f = lambda t, hh: torch.func.functional_call(net, dict(zip([k for k, _ in net.named_parameters()], ps)), (t, hh))  # noqa: E731
        return I.aten_curve(f, x0, x, h, 7)

    assert torch.autograd.gradcheck(fn, (x0, x, h, *params), eps=1e-6, atol=1e-6, rtol=1e-5)


def test_gradients_reach_every_parameter_and_match_float64():
    i = 1
    model, x, h = C.build(C.CASES[i])
    T = C.case_truth(i)
    xr, hr = x.clone().requires_grad_(), h.clone().requires_grad_()
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        t, y = model.forward_curve(xr, hr)
    (y * T.G.float()).sum().backward()
    assert U.scaled_err(xr.grad.numpy(), T.dx) <= C.TOL and U.scaled_err(hr.grad.numpy(), T.dh) <= C.TOL
    assert all(p.grad is not None and bool(p.grad.abs().sum() > 0) for p in model.parameters())


# ---- cumulative incidence -----------------------------------------------------------------------------------------------------------
def test_cumulative_incidence_against_nested_composite_quadrature():
    c = C.CIF_CASE
    model, x, h = C.build(c)
    m64, x64, h64 = copy.deepcopy(model).double(), x.double().abs() + 0.5, h.double()
    with torch.no_grad():
        t, cif = m64.cumulative_incidence(x64, h64, curve=True)
        end = m64.cumulative_incidence(x64, h64)
    assert cif.shape == (4, 51, 2) and end.shape == (4, 2) and torch.equal(end, cif[:, -1]) and torch.equal(cif[:, 0], torch.zeros(4, 2, dtype=torch.float64))
    ref = C.cif_composite(m64, x64, h64, t)
    sep = C.cif_separate(m64, x64, h64, t, c.nb_steps)
    err_sep, err = float((sep - ref).abs().max()), float((cif - ref).abs().max())
    print(f"CIF: separate 50-node nested quadratures vs composite {err_sep:.2e}; the curve vs composite {err:.2e}")
    assert 0 < err_sep < 1e-3                       # (the composite rule resolves what the 50-node rule misses)
    assert err <= 2 * err_sep
    assert bool((cif[:, 1:] > cif[:, :-1]).all())                                          # increasing in t
    # the float32 model agrees with the float64 one to arithmetic
    with torch.no_grad(), warnings.catch_warnings():
        warnings.simplefilter("ignore")
        cif32 = model.cumulative_incidence(x64.float(), h, curve=True)[1]
    assert U.rel_err(cif32.numpy(), cif.numpy()) <= C.TOL


def test_cumulate_is_differentiable_and_checks_shapes():
    v = torch.rand(3, 8, 2, dtype=torch.float64, requires_grad=True)
    x = torch.rand(3, 1, dtype=torch.float64) + 0.5
    assert torch.autograd.gradcheck(lambda v: I.cumulate(v, None, x, 7), (v,))
    with pytest.raises(RuntimeError, match="cumulate takes values"):
        I.cumulate(torch.rand(3, 7, 2), None, torch.rand(3, 1), 7)


# ---- the ops ---------------------------------------------------------------------------------------------------------------------------
def _fake_args(dev="cuda", K=3, n=7, B=5, E=2, dtype=torch.float32):
    W = [torch.empty(16, 1 + E, device=dev), torch.empty(16, 16, device=dev), torch.empty(K, 16, device=dev)]
    b = [torch.empty(16, device=dev), torch.empty(16, device=dev), torch.empty(K, device=dev)]
    return dict(x0=None, x=torch.empty(B, 1, device=dev, dtype=dtype), h=torch.empty(B, E, device=dev, dtype=dtype), W=W, b=b)


def _nodes(a, n=7):
    return torch.ops.umnn.cc_forward_multi_nodes(a["x0"], a["x"], a["h"], a["W"], a["b"], 1, 0, n)


def test_op_fakes_give_shapes_and_refuse_wrong_device_dtype_and_shape():
    from torch._subclasses.fake_tensor import FakeTensorMode
    assert {"cc_forward_multi_nodes", "cc_cumulate"} <= set(ops.OPS)
    with FakeTensorMode():
        a = _fake_args()
        F, fn = _nodes(a)
        assert F.shape == (5, 3) and fn.shape == (5, 8, 3) and fn.dtype == torch.float32
        assert _nodes(_fake_args(K=1))[1].shape == (5, 8, 1)                       # a single output is taken here
        out = torch.ops.umnn.cc_cumulate(fn, None, a["x"], 7)
        assert out.shape == (5, 8, 3) and torch.ops.umnn.cc_cumulate(fn, a["x"], a["x"], 7, True).shape == (5, 8, 3)
        for bad, msg in ((_fake_args(dev="cpu"), "CUDA"), (_fake_args(dtype=torch.float64), "dtype"), (_fake_args(K=17), "n_out"),
                         (dict(_fake_args(), x=torch.empty(5, 2, device="cuda")), r"\[B, 1\]"),
                         (dict(_fake_args(), h=torch.empty(5, 3, device="cuda")), "h has shape"),
                         (dict(_fake_args(), x0=torch.empty(4, 1, device="cuda")), "x0 has shape")):
            with pytest.raises(RuntimeError, match=msg):
                _nodes(bad)
        x = a["x"]
        for v, xx, x0, n, msg in ((fn.cpu(), x.cpu(), None, 7, "CUDA"), (fn.double(), x, None, 7, "dtype"), (fn, x, None, 8, "values has shape"),
                                  (fn[:, :, 0], x, None, 7, "values has shape"), (fn, x[:4], None, 7, "x has shape"),
                                  (fn, x, x[:4], 7, "x0 has shape"), (torch.empty(5, 8, 17, device="cuda"), x, None, 7, "K = 17"),
                                  (fn, x.cpu(), None, 7, "x is on")):
            with pytest.raises(RuntimeError, match=msg):
                torch.ops.umnn.cc_cumulate(v, x0, xx, n)
