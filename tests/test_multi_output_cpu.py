"""Multi-output MonotonicNN without a GPU: the constructor and its n_out = 1 identity, the ATen implementation against the float64
truth, spec recognition and the refusals of the single-output consumers, ``inverse(..., output=k)``, and the C ABI's argument checks.

Truth and tolerance (1e-5): tests/_multi_output_cases.py."""
import copy
import ctypes
import warnings

import numpy as np
import pytest
import torch

import umnn_amd
from tests import _multi_output_cases as M
from tests import _util as U
from umnn_amd import _lib, integral as I
from umnn_amd.nets import IntegrandNetwork, IntegrandNN, mlp_spec

TOL = M.TOL


@pytest.fixture(autouse=True)
def _quiet():
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        yield


def _data(B, E, K, seed):
    gen = torch.Generator().manual_seed(seed)
    return torch.randn(B, 1, generator=gen) * 2, torch.randn(B, E, generator=gen), torch.randn(B, K, generator=gen)


def _all_grads(m, x, h, gy):
    m.zero_grad()
    xr, hr = x.clone().requires_grad_(), h.clone().requires_grad_()
    y = m(xr, hr)
    (y * gy).sum().backward()
    return y.detach(), xr.grad, hr.grad, [p.grad.clone() for p in m.parameters()]


# ------------------------------------------------------------------------------------------------------------ constructor
def test_n_out_one_is_the_model_of_today():
    torch.manual_seed(0)
    a = umnn_amd.MonotonicNN(3, [16, 16])
    torch.manual_seed(0)
    b = umnn_amd.MonotonicNN(3, [16, 16], n_out=1)
    sa, sb = a.state_dict(), b.state_dict()
    assert list(sa) == list(sb)
    assert list(sa) == ["integrand.net.0.weight", "integrand.net.0.bias", "integrand.net.2.weight", "integrand.net.2.bias",
                        "integrand.net.4.weight", "integrand.net.4.bias", "net.0.weight", "net.0.bias", "net.2.weight", "net.2.bias",
                        "net.4.weight", "net.4.bias"]
    assert all(sa[k].shape == sb[k].shape and torch.equal(sa[k], sb[k]) for k in sa)
    assert sa["integrand.net.4.weight"].shape == (1, 16) and sa["net.4.weight"].shape == (2, 16)
    x, h, gy = _data(21, 2, 1, 3)
    for u, v in zip(_all_grads(a, x, h, gy)[:3], _all_grads(b, x, h, gy)[:3]):
        assert u.shape == v.shape and torch.equal(u, v)
    for u, v in zip(_all_grads(a, x, h, gy)[3], _all_grads(b, x, h, gy)[3]):
        assert torch.equal(u, v)


def test_signature_keeps_the_reference_order():
    import inspect
    assert list(inspect.signature(umnn_amd.MonotonicNN.__init__).parameters) == ["self", "in_d", "hidden_layers", "nb_steps", "dev", "n_out"]
    assert list(inspect.signature(IntegrandNN.__init__).parameters) == ["self", "in_d", "hidden_layers", "n_out"]
    m = umnn_amd.MonotonicNN(3, [8, 8], 20, "cpu", 3)
    assert m.n_out == 3 and m.net[-1].out_features == 6 and m.integrand.net[-2].out_features == 3


# ------------------------------------------------------------------------------------------------------------ ATen = the truth
def _mono64(m64, x, h):
    out = m64.net(h)
    K = m64.n_out
    F = M.quadrature64(m64.integrand, torch.zeros_like(x), x, h, m64.nb_steps)
    return torch.exp(out[:, K:]) * F + out[:, :K]


def test_three_outputs_match_float64_and_three_single_models():
    torch.manual_seed(1)
    m = umnn_amd.MonotonicNN(3, [20, 20], nb_steps=30, n_out=3)
    x, h, gy = _data(29, 2, 3, 5)
    y, dx, dh, dps = _all_grads(m, x, h, gy)
    assert y.shape == (29, 3) and I.path_taken() == "aten" and I.backward_path_taken() == "aten"

    m64 = copy.deepcopy(m).double()
    x64, h64 = x.double().requires_grad_(), h.double().requires_grad_()
    y64 = _mono64(m64, x64, h64)
    (y64 * gy.double()).sum().backward()
    with torch.no_grad():       # d/dx by the operator's convention: the Leibniz term, y_k' = exp(s_k) f_k(x)
        dx64 = (torch.exp(m64.net(h64)[:, 3:]) * m64.integrand(x64, h64) * gy.double()).sum(1, keepdim=True)
    lins = [l for l in m.integrand.net if isinstance(l, torch.nn.Linear)]
    margin = U.kink_margin(M.O.Net([l.weight.detach().double().numpy() for l in lins], [l.bias.detach().double().numpy() for l in lins],
                                   M.O.RELU, M.O.ELU1), np.zeros((29, 1)), x.numpy(), h.numpy(), 30)
    assert margin >= M.MIN_MARGIN
    assert U.rel_err(y.numpy(), y64.detach().numpy()) <= TOL
    assert U.scaled_err(dx.numpy(), dx64.numpy()) <= TOL
    assert U.scaled_err(dh.numpy(), h64.grad.numpy()) <= TOL
    for (name, p), p64 in zip(m.named_parameters(), m64.parameters()):
        assert U.scaled_err(dps.pop(0).numpy(), p64.grad.numpy()) <= TOL, name

    # ... and three single-output models that share the hidden weights and take row k of the last layers
    for k in range(3):
        s = umnn_amd.MonotonicNN(3, [20, 20], nb_steps=30)
        sd = {n: v.clone() for n, v in m.state_dict().items()}
        sd["integrand.net.4.weight"], sd["integrand.net.4.bias"] = sd["integrand.net.4.weight"][k:k + 1], sd["integrand.net.4.bias"][k:k + 1]
        sd["net.4.weight"], sd["net.4.bias"] = sd["net.4.weight"][[k, 3 + k]], sd["net.4.bias"][[k, 3 + k]]
        s.load_state_dict(sd)
        with torch.no_grad():
            assert U.rel_err(s(x, h).numpy(), y[:, [k]].numpy()) <= TOL


@pytest.mark.parametrize("i", [0, 4])
def test_operator_cases_on_aten(i):
    """Cases 0 (K = 2) and 4 (K = 17: no spec, the integrand is just a callable) through ParallelNeuralIntegral on CPU tensors."""
    c = M.CASES[i]
    net, x, h, g = M.build(c)
    T = M.case_truth(i)
    assert T.margin >= M.MIN_MARGIN
    xr, hr = x.clone().requires_grad_(), h.clone().requires_grad_()
    F = I.ParallelNeuralIntegral.apply(torch.zeros_like(xr), xr, net, I._flatten(net.parameters()), hr, c.nb_steps)
    (F * g).sum().backward()
    assert F.shape == (c.B, c.K) and xr.grad.shape == (c.B, 1) and I.path_taken() == "aten"
    assert U.rel_err(F.detach().numpy(), T.F) <= TOL
    assert U.scaled_err(xr.grad.numpy(), T.dx) <= TOL and U.scaled_err(hr.grad.numpy(), T.dh) <= TOL
    for p, t in zip(net.parameters(), T.dparams):
        assert U.scaled_err(p.grad.numpy(), t) <= TOL


# ------------------------------------------------------------------------------------------------------------ specs and refusals
def test_spec_recognises_the_output_width():
    spec = mlp_spec(IntegrandNN(3, [20, 20], n_out=4))
    assert spec is not None and spec.linears[-1].out_features == 4 and umnn_amd.nets.n_out_of(spec) == 4
    spec = mlp_spec(IntegrandNetwork(nnets=1, nin=3, hidden_sizes=[20, 33, 17], nout=5, act_func="Sigmoid"))
    assert spec is not None and umnn_amd.nets.n_out_of(spec) == 5 and spec.out_act == _lib.OUT_SIGMOID
    assert umnn_amd.nets.n_out_of(mlp_spec(IntegrandNN(3, [20, 20]))) == 1
    assert mlp_spec(IntegrandNN(3, [20, 20], n_out=16)) is not None
    assert mlp_spec(IntegrandNN(3, [20, 20], n_out=17)) is None


def test_single_output_consumers_refuse_by_name():
    net = IntegrandNN(3, [20, 20], n_out=4)
    x, h, _ = _data(8, 2, 4, 1)
    flat = I._flatten(net.parameters())
    with pytest.raises(RuntimeError, match="n_out"):
        I.IntegralWithJacobian.apply(torch.zeros_like(x), x, net, flat, h, 20)
    with pytest.raises(RuntimeError, match="n_out"):
        I.InverseNeuralIntegral.apply(x, net, flat, h, 20)
    # a flow block handed a multi-output integrand
    torch.manual_seed(0)
    flow = umnn_amd.UMNNMAFFlow(nb_flow=1, nb_in=2, hidden_derivative=[20, 20], hidden_embedding=[16, 16], embedding_s=2, nb_steps=20,
                                solver="CCParallel")
    flow.nets[0].net.parallel_nets = IntegrandNetwork(2, 3, [20, 20], 4)
    with pytest.raises(RuntimeError, match="n_out"):
        flow.compute_ll(torch.randn(8, 2))
    from umnn_amd.nets import single_spec
    with pytest.raises(RuntimeError, match="n_out"):
        single_spec(net, "the flow inverse")


def test_more_than_one_dimension_raises():
    net = IntegrandNN(3, [20, 20], n_out=3)
    x = torch.randn(8, 2)
    h = torch.randn(8, 4)
    with pytest.raises(RuntimeError, match=r"n_out = 3.*\[B, 1\]"):
        I.ParallelNeuralIntegral.apply(torch.zeros_like(x), x, net, I._flatten(net.parameters()), h, 20)
    with pytest.raises(RuntimeError, match="n_out = 3"):
        I.NeuralIntegral.apply(torch.zeros_like(x), x, net, I._flatten(net.parameters()), h, 20)
    with pytest.raises(RuntimeError, match="n_out = 3"):
        I.integrate(torch.zeros_like(x), 20, x / 20, net, h)


# ------------------------------------------------------------------------------------------------------------ inverse
def test_inverse_of_one_output():
    torch.manual_seed(2)
    K, k = 3, 1
    m = umnn_amd.MonotonicNN(3, [20, 20], nb_steps=30, n_out=K).double()
    gen = torch.Generator().manual_seed(9)
    x = torch.randn(17, 1, generator=gen, dtype=torch.float64) * 2
    h = torch.randn(17, 2, generator=gen, dtype=torch.float64)
    with torch.no_grad():
        y = m(x, h)[:, [k]]
    yr, hr = y.clone().requires_grad_(), h.clone().requires_grad_()
    m.zero_grad()
    xi, fx, status = m.inverse(yr, hr, tol=1e-13, return_info=True, output=k)
    assert int((status & (umnn_amd.SOLVE_CAPPED | umnn_amd.SOLVE_NONFINITE | umnn_amd.SOLVE_CLAMPED)).max()) == 0
    with torch.no_grad():
        back = m(xi.detach(), h)[:, [k]]
    assert U.rel_err(back.numpy(), y.numpy()) <= 1e-10          # the solve's tolerance (1e-13 on t) with room for exp(s)
    assert U.rel_err(xi.detach().numpy(), x.numpy()) <= 1e-9
    gx = torch.randn(17, 1, generator=gen, dtype=torch.float64)
    (xi * gx).sum().backward()

    # implicit-function truth in float64: G(x, y, h, theta) = y_k(x, h; theta) - y = 0  =>  dx = -(dG/dx)^-1 dG/d(.), with dG/dx the
    # operator's own derivative exp(s_k) f_k(x) (the Leibniz term)
    m2 = copy.deepcopy(m)
    m2.zero_grad()
    h2 = h.clone().requires_grad_()
    xs = xi.detach()
    with torch.no_grad():
        slope = torch.exp(m2.net(h)[:, [K + k]]) * m2.integrand(xs, h)[:, [k]]
    out = m2.net(h2)
    yk = torch.exp(out[:, [K + k]]) * M.quadrature64(m2.integrand, torch.zeros_like(xs), xs, h2, 30)[:, [k]] + out[:, [k]]
    (yk * (-gx / slope)).sum().backward()
    assert U.scaled_err(yr.grad.numpy(), (gx / slope).numpy()) <= 1e-9
    assert U.scaled_err(hr.grad.numpy(), h2.grad.numpy()) <= 1e-9
    for (name, p), q in zip(m.named_parameters(), m2.parameters()):
        assert p.grad is not None, name
        assert U.scaled_err(p.grad.numpy(), q.grad.numpy()) <= 1e-9, name
    last = m.integrand.net[-2]
    rows = [r for r in range(K) if r != k]
    assert torch.count_nonzero(last.weight.grad[rows]) == 0 and torch.count_nonzero(last.bias.grad[rows]) == 0
    assert torch.count_nonzero(last.weight.grad[k]) > 0
    with pytest.raises(IndexError):
        m.inverse(y, h, output=3)


# ------------------------------------------------------------------------------------------------------------ C ABI
def _desc(widths, ptr=0x1000):
    d = _lib.MlpDesc()
    d.n_linear = len(widths) - 1
    for i, w in enumerate(widths):
        d.widths[i] = w
    for l in range(d.n_linear):
        d.W[l], d.b[l] = ptr, ptr
    return d


def test_abi_symbols_and_argument_checks():
    handle = ctypes.CDLL(_lib.LIB_PATH)
    for name in ("umnn_cc_forward_multi", "umnn_cc_backward_multi", "umnn_cc_backward_multi_workspace_bytes"):
        assert hasattr(handle, name) and name in _lib.SIGNATURES
    lib = _lib.lib()
    p = ctypes.c_void_p(0x1000)
    four = _desc([3, 16, 16, 4])
    # every single-output entry point keeps its check and its message
    rc = lib.umnn_cc_forward(ctypes.byref(four), None, p, p, p, p, 20, 4, 1, 2, 0, p, None, None, None)
    assert rc == _lib.EINVAL and lib.umnn_last_error() == b"integrand output width must be 1"
    assert lib.umnn_cc_backward_workspace_bytes(ctypes.byref(four), 4, 1, 2) == -1
    # the multi entries: K = 17 and K = 0 are errors with a message; K = 1 belongs to the single-output entries
    for K in (17, 0, 1):
        bad = _desc([3, 16, 16, K])
        rc = lib.umnn_cc_forward_multi(ctypes.byref(bad), None, p, p, p, p, 20, 4, 1, 2, 0, p, None, None, None)
        assert rc == _lib.EINVAL and b"output width" in lib.umnn_last_error(), K
        rc = lib.umnn_cc_backward_multi(ctypes.byref(bad), None, p, p, p, p, p, 20, 4, 1, 2, 0, None, None, None, None, p, 1 << 20, None)
        assert rc == _lib.EINVAL and b"output width" in lib.umnn_last_error(), K
        assert lib.umnn_cc_backward_multi_workspace_bytes(ctypes.byref(bad), 4, 1, 2) == -1
    # valid descriptor: empty batch is a no-op, null inputs are named, the workspace size needs no device
    assert lib.umnn_cc_forward_multi(ctypes.byref(four), None, p, p, p, p, 20, 0, 1, 2, 0, p, None, None, None) == 0
    rc = lib.umnn_cc_forward_multi(ctypes.byref(four), None, None, p, p, p, 20, 4, 1, 2, 0, p, None, None, None)
    assert rc == _lib.EINVAL and b"non-null" in lib.umnn_last_error()
    assert lib.umnn_cc_backward_multi_workspace_bytes(ctypes.byref(four), 64, 1, 2) > 0
    assert lib.umnn_cc_backward_multi_workspace_bytes(ctypes.byref(four), 0, 1, 2) == 0
    # images beyond the LDS: UMNN_EUNSUPPORTED (the host then integrates on ATen)
    deep = _desc([3, 127, 127, 127, 127, 127, 127, 5])
    rc = lib.umnn_cc_forward_multi(ctypes.byref(deep), None, p, p, p, p, 20, 4, 1, 2, 0, p, None, None, None)
    assert rc == _lib.EUNSUPPORTED and b"LDS" in lib.umnn_last_error()
