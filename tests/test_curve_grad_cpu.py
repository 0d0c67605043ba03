"""The backward of the curves on the CPU: the adjoint table, the decomposition of the gradient (``curve_vjp`` on
``aten_cumulate_adjoint`` and ``aten_vjp_nodes``, the ATen mirrors of the two HIP entries) against the float64 truth, and
``backward="hip"`` on what the kernels do not take -- host tensors, K = 17 -- being the ATen path bit for bit.  Cases, truth and
tolerance: tests/_curve_grad_cases.py."""
import ctypes
import warnings

import numpy as np
import pytest
import torch

import umnn_amd
from tests import _curve_cases as C
from tests import _curve_grad_cases as G
from tests import _util as U
from umnn_amd import _lib, integral as I
from umnn_amd import ops
from umnn_amd.quadrature import cc_cumulative_matrix, device_cumulative_adjoint, device_cumulative_matrix


def _errs(got, T):
    """{name: scaled_err} of (dx, dh, {parameter: grad}) against a GradTruth."""
    dx, dh, dparams = got
    out = {"dx": U.scaled_err(dx.numpy(), T.dx), "dh": U.scaled_err(dh.numpy(), T.dh)}
    for k, v in dparams.items():
        out[k] = U.scaled_err(v.numpy(), T.dparams[k])
    return out


# ---- the table --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 2, 7, 8, 20, 50, 51, 100])
def test_adjoint_table_is_the_cumulative_matrix_transposed(n):
    Q = cc_cumulative_matrix(n)
    a, b = device_cumulative_adjoint(n, "cpu"), device_cumulative_adjoint(n, "cpu", ascending=True)
    assert a.dtype == torch.float32 and a.is_contiguous() and device_cumulative_adjoint(n, "cpu") is a
    assert np.array_equal(a.numpy(), Q[::-1, :].T.astype(np.float32))                     # out in node order, g ascending
    assert np.array_equal(b.numpy(), Q[::-1, ::-1].T.astype(np.float32))                  # out ascending, g ascending
    # ... which are the transposes of what the forward applies (its output index reversed), entry for entry
    assert torch.equal(a, device_cumulative_matrix(n, "cpu").flip(0).t())
    assert torch.equal(b, device_cumulative_matrix(n, "cpu", ascending=True).flip(0).t())
    assert device_cumulative_adjoint(n, "cpu", dtype=torch.float64).dtype == torch.float64
    # existing calls return what they returned
    assert np.array_equal(device_cumulative_matrix(n, "cpu").numpy(), Q.astype(np.float32))


def test_adjoint_einsum_is_the_adjoint_of_aten_cumulate():
    n, B, K = 9, 5, 3
    g = torch.Generator().manual_seed(0)
    v, x0, x = torch.randn(B, n + 1, K, generator=g, dtype=torch.float64), torch.randn(B, 1, generator=g, dtype=torch.float64), \
        torch.randn(B, 1, generator=g, dtype=torch.float64)
    gC = torch.randn(B, n + 1, K, generator=g, dtype=torch.float64)
    for ascending in (False, True):
        vr = v.clone().requires_grad_()
        (I.aten_cumulate(vr, x0, x, n, ascending) * gC).sum().backward()
        a = I.aten_cumulate_adjoint(gC, n, ascending) * ((x - x0) / 2).unsqueeze(2)
        assert U.scaled_err(a.numpy(), vr.grad.numpy()) <= 1e-14


# ---- the decomposition ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("i", G.HIP_CASES)
def test_decomposition_matches_float64(i):
    """Adjoint table, glue and ``aten_vjp_nodes`` in float32 -- the arithmetic of the HIP backward, on ATen -- against the truth; the
    float32 ATen curve under autograd next to it, for the headroom figure."""
    model, x, h = G.build(i)
    T = G.case_truth(i)
    n, K = model.nb_steps, model.n_out
    G32 = G.on(G.cotangents(x.shape[0], n, K), x)
    names = [k for k, _ in model.named_parameters()]
    # (a) autograd through aten_curve
    xr, hr = x.clone().requires_grad_(), h.clone().requires_grad_()
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        out = model.forward_curve(xr, hr, with_derivative=True)
    grads = torch.autograd.grad(G.loss_of(out, G32), [xr, hr] + list(model.parameters()))
    auto = _errs((grads[0], grads[1], dict(zip(names, grads[2:]))), T)
    # (b) the decomposition: the conditioner by autograd, the curve by curve_vjp
    xr, hr = x.clone().requires_grad_(), h.clone().requires_grad_()
    with torch.no_grad():
        t, Cv, f = I.aten_curve(model.integrand, torch.zeros_like(x), x, h, n)
    tt, CC, ff = (v.clone().requires_grad_() for v in (t, Cv, f))
    o, ls = model._offset_log_scaling(hr)
    sc = torch.exp(ls).unsqueeze(1)
    loss = G.loss_of((tt, sc * CC + o.unsqueeze(1), sc * ff), G32)
    cond = [p for k, p in model.named_parameters() if k.startswith("net.")]
    gt, gC, gf, dh_cond, *dcond = torch.autograd.grad(loss, [tt, CC, ff, hr] + cond)
    with torch.no_grad():
        _, dx, dh, dtheta = I.curve_vjp(None, x, f.flip(1).contiguous(), gt, gC, gf, n, [False, True, True, True],
                                        lambda g: I.aten_cumulate_adjoint(g, n),
                                        lambda cot: I.aten_vjp_nodes(model.integrand, torch.zeros_like(x), x, h, cot, n))
    dparams = dict(zip([k for k in names if k.startswith("net.")], dcond))
    dparams.update(zip([k for k in names if k.startswith("integrand.")],
                       I.split_flat(dtheta, [p.shape for p in model.integrand.parameters()], [True] * 99)))
    dec = _errs((dx, dh + dh_cond, dparams), T)
    worst = lambda e: max(v for k, v in e.items() if k not in ("dx", "dh"))      # noqa: E731
    print(f"case {i}: autograd dx {auto['dx']:.2e} dh {auto['dh']:.2e} param {worst(auto):.2e}; "
          f"decomposition dx {dec['dx']:.2e} dh {dec['dh']:.2e} param {worst(dec):.2e}; margin {T.margin:.2e}")
    assert T.margin >= G.MIN_MARGIN
    assert set(dec) == set(auto) == {"dx", "dh", *names}
    for k, v in dec.items():
        assert v <= G.TOL, (k, v)
    for k, v in auto.items():
        assert v <= G.TOL, (k, v)


def test_decomposition_with_nonzero_x0_matches_float64():
    net, x0, x, h, n = G.x0_case()
    T = G.x0_truth()
    G32 = G.on(G.cotangents(x.shape[0], n, C.X0_CASE.K), x)
    with torch.no_grad():
        f = I.aten_curve(net, x0, x, h, n)[2]
        dx0, dx, dh, dtheta = I.curve_vjp(x0, x, f.flip(1).contiguous(), G32[2], G32[0], G32[1], n, [True] * 4,
                                          lambda g: I.aten_cumulate_adjoint(g, n), lambda cot: I.aten_vjp_nodes(net, x0, x, h, cot, n))
    flat = np.concatenate([T.dparams[k].reshape(-1) for k, _ in net.named_parameters()])
    errs = [U.scaled_err(a.numpy(), b) for a, b in ((dx0, T.dx0), (dx, T.dx), (dh, T.dh), (dtheta, flat))]
    print(f"x0 != 0: dx0 {errs[0]:.2e} dx {errs[1]:.2e} dh {errs[2]:.2e} dtheta {errs[3]:.2e}; margin {T.margin:.2e}")
    assert T.margin >= G.MIN_MARGIN and bool((x[0] == x0[0]).all()) and max(errs) <= G.TOL


# ---- the switch on what the kernels do not take --------------------------------------------------------------------------------------
def _grads(model, x, h, backward):
    model.zero_grad()
    xr, hr = x.clone().requires_grad_(), h.clone().requires_grad_()
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        out = model.forward_curve(xr, hr, with_derivative=True, backward=backward)
        cif = model.cumulative_incidence(xr, hr, backward=backward)
    path = I.path_taken()
    (G.loss_of(out, G.on(G.cotangents(x.shape[0], model.nb_steps, model.n_out), x)) + cif.sum()).backward()
    return path, list(out) + [cif, xr.grad, hr.grad] + [p.grad.clone() for p in model.parameters()]


@pytest.mark.parametrize("i", [1, 4])
def test_hip_switch_on_host_tensors_and_k17_is_the_aten_path_bit_for_bit(i):
    model, x, h = G.build(i)
    pa, a = _grads(model, x, h, "aten")
    ph, b = _grads(model, x, h, "hip")
    assert pa == ph == "aten" and I.backward_path_taken() in (None, "aten")
    for u, v in zip(a, b):
        assert torch.equal(u, v)
    with pytest.raises(ValueError):
        model.forward_curve(x, h, backward="triton")


def test_cumulate_hip_switch_on_host_tensors_matches_autograd_of_aten_cumulate():
    n, B, K = 20, 6, 3
    g = torch.Generator().manual_seed(1)
    v, x0, x = (torch.randn(s, generator=g) for s in ((B, n + 1, K), (B, 1), (B, 1)))
    gC = torch.randn(B, n + 1, K, generator=g)
    want = None
    for backward, x0_ in (("aten", x0), ("hip", x0), ("hip", None)):
        leaves = [t.clone().requires_grad_() for t in ((v, x) if x0_ is None else (v, x, x0_))]
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            out = umnn_amd.integral.cumulate(leaves[0], None if x0_ is None else leaves[2], leaves[1], n, backward=backward)
        ref = I.aten_cumulate(*(t.detach() for t in (leaves[0], torch.zeros_like(x) if x0_ is None else leaves[2], leaves[1])), n)
        assert torch.equal(out, ref) and I.path_taken() == "aten"
        grads = torch.autograd.grad((out * gC).sum(), leaves)
        if want is None:
            want = grads
        elif x0_ is not None:
            assert all(torch.equal(a, b) for a, b in zip(grads, want))
        # the formulas of the HIP backward (CumulateFunction), on the ATen adjoint
        vv, xx = leaves[0].detach(), leaves[1].detach()
        span = xx if x0_ is None else xx - leaves[2].detach()
        a = I.aten_cumulate_adjoint(gC, n, ascending=True)
        dx = (a * vv).sum((1, 2)).unsqueeze(1) / 2
        assert U.scaled_err((a * (span / 2).unsqueeze(2)).numpy(), grads[0].numpy()) <= 1e-6
        assert U.scaled_err(dx.numpy(), grads[1].numpy()) <= 1e-6
        if x0_ is not None:
            assert U.scaled_err(-dx.numpy(), grads[2].numpy()) <= 1e-6


# ---- C ABI and ops ----------------------------------------------------------------------------------------------------------------
def _desc(widths):
    d = _lib.MlpDesc()
    d.n_linear = len(widths) - 1
    for i, w in enumerate(widths):
        d.widths[i] = w
    for l in range(d.n_linear):
        d.W[l], d.b[l] = 0x1000, 0x1000                     # (never read: no call below launches)
    d.hidden_act, d.out_act = _lib.ACT_RELU, _lib.OUT_ELU_PLUS_ONE
    return d


def test_new_entries_answer_without_a_device():
    handle = ctypes.CDLL(_lib.LIB_PATH)
    for name in ("umnn_cc_backward_multi_nodes", "umnn_cc_backward_multi_nodes_workspace_bytes", "umnn_cc_cumulate_adjoint"):
        assert hasattr(handle, name) and name in _lib.SIGNATURES
    lib = _lib.lib()
    p = ctypes.c_void_p(0x1000)

    def bwd(desc, n=20, B=0, d=1, cot=None):
        return lib.umnn_cc_backward_multi_nodes(ctypes.byref(desc), None, None, None, cot, None, n, B, d, 2, None, None, None, None, None, 0, None)

    for K in (1, 2, 16):                                    # zero rows: the checks of the net, nothing to launch
        assert bwd(_desc([3, 16, 16, K])) == 0
        assert lib.umnn_cc_backward_multi_nodes_workspace_bytes(ctypes.byref(_desc([3, 16, 16, K])), 64, 2) > 0
    four = _desc([3, 16, 16, 4])
    assert lib.umnn_cc_backward_multi_nodes_workspace_bytes(ctypes.byref(four), 64, 2) == \
        lib.umnn_cc_backward_multi_workspace_bytes(ctypes.byref(four), 64, 1, 2)
    assert lib.umnn_cc_backward_multi_workspace_bytes(ctypes.byref(_desc([3, 16, 16, 1])), 64, 1, 2) == -1      # (as before)
    for K in (0, 17):
        assert bwd(_desc([3, 16, 16, K])) == _lib.EINVAL and b"output width" in lib.umnn_last_error()
    assert bwd(four, d=2) == _lib.EINVAL and b"d must be 1" in lib.umnn_last_error()
    assert bwd(four, n=0) == _lib.EINVAL and b"nb_steps" in lib.umnn_last_error()
    assert bwd(four, B=4) == _lib.EINVAL and b"non-null" in lib.umnn_last_error()
    assert bwd(four, B=4, cot=p) == _lib.EINVAL and b"non-null" in lib.umnn_last_error()
    deep = _desc([3, 127, 127, 127, 127, 127, 127, 5])
    assert bwd(deep) == _lib.EUNSUPPORTED and bwd(_desc([3, 127, 127, 127, 5])) == _lib.EUNSUPPORTED
    # the adjoint cumulate: the limits and answers of umnn_cc_cumulate
    assert lib.umnn_cc_cumulate_adjoint(None, None, 127, 0, 16, None, None) == 0
    assert lib.umnn_cc_cumulate_adjoint(None, None, 128, 0, 2, None, None) == _lib.EUNSUPPORTED
    assert lib.umnn_cc_cumulate_adjoint(None, None, 0, 0, 2, None, None) == _lib.EINVAL
    assert lib.umnn_cc_cumulate_adjoint(None, None, 20, 0, 17, None, None) == _lib.EINVAL
    assert lib.umnn_cc_cumulate_adjoint(None, p, 20, 4, 2, p, None) == _lib.EINVAL and b"non-null" in lib.umnn_last_error()


def test_ops_are_registered_and_their_fakes_give_shapes_and_refuse():
    from torch._subclasses.fake_tensor import FakeTensorMode
    assert {"cc_backward_multi_nodes", "cc_cumulate_adjoint"} <= set(ops.OPS)
    assert hasattr(torch.ops.umnn, "cc_backward_multi_nodes") and hasattr(torch.ops.umnn, "cc_cumulate_adjoint")
    with FakeTensorMode():
        B, E, n = 5, 2, 7
        for K in (1, 3):
            W = [torch.empty(16, 1 + E, device="cuda"), torch.empty(16, 16, device="cuda"), torch.empty(K, 16, device="cuda")]
            b = [torch.empty(w.shape[0], device="cuda") for w in W]
            x, h, cot = torch.empty(B, 1, device="cuda"), torch.empty(B, E, device="cuda"), torch.empty(B, n + 1, K, device="cuda")
            out = torch.ops.umnn.cc_backward_multi_nodes(None, x, h, cot, W, b, 1, 0, n, [True, True, True, False])
            assert [tuple(t.shape) for t in out] == [(0,), (B, 1), (B, E), (0,)]           # (no x0: no d_x0)
            out = torch.ops.umnn.cc_backward_multi_nodes(x, x, h, cot, W, b, 1, 0, n, [True, False, False, True])
            assert [tuple(t.shape) for t in out] == [(B, 1), (0,), (0,), (sum(w.numel() for w in W) + sum(v.numel() for v in b),)]
            assert torch.ops.umnn.cc_cumulate_adjoint(cot, n).shape == cot.shape
            assert torch.ops.umnn.cc_cumulate_adjoint(cot, n, True).shape == cot.shape
        for bad, msg in ((dict(cot=cot[:, :7]), "cot_nodes has shape"), (dict(cot=cot.double()), "dtype"), (dict(cot=cot.cpu()), "cot_nodes is on"),
                         (dict(need=[True] * 3), "need has 3"), (dict(x=torch.empty(B, 2, device="cuda")), r"\[B, 1\]")):
            kw = dict(dict(x=x, cot=cot, need=[True] * 4), **bad)
            with pytest.raises(RuntimeError, match=msg):
                torch.ops.umnn.cc_backward_multi_nodes(None, kw["x"], h, kw["cot"], W, b, 1, 0, n, kw["need"])
        for g, steps, msg in ((cot.cpu(), n, "CUDA"), (cot.double(), n, "dtype"), (cot, n + 1, "g has shape"), (cot[:, :, 0], n, "g has shape"),
                              (torch.empty(B, n + 1, 17, device="cuda"), n, "K = 17")):
            with pytest.raises(RuntimeError, match=msg):
                torch.ops.umnn.cc_cumulate_adjoint(g, steps)
