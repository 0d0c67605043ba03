"""Multi-output quadrature on the GPU (csrc/cc_multi.hip): forward, column identity with the single-output fp32 kernel, backward,
the n_out > 16 ATen route, MonotonicNN(n_out=K) end to end, graph mode, and the C ABI at d = 3.

Truth, tolerance (1e-5: ``rel_err`` for values, ``scaled_err`` for gradients), kink margins (>= 1e-6, no row excluded) and the
five cases: tests/_multi_output_cases.py."""
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
from umnn_amd.nets import IntegrandNetwork, MlpSpec, TensorLinear, mlp_spec

pytestmark = pytest.mark.gpu
TOL = M.TOL
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


def _kname():
    return _lib.lib().umnn_last_kernel_name().decode()


def _apply(net, x, h, nb_steps, x0=None, inv_f=False):
    x0 = torch.zeros_like(x) if x0 is None else x0
    return I.ParallelNeuralIntegral.apply(x0, x, net, I._flatten(net.parameters()), h, nb_steps, inv_f)


def _on(dev, net, *tensors):
    return (copy.deepcopy(net).to(dev),) + tuple(t.to(dev) for t in tensors)


# ------------------------------------------------------------------------------------------------------------ forward
@pytest.mark.parametrize("i", [0, 1, 2, 3])
def test_forward_matches_float64(dev, i):
    c = M.CASES[i]
    net, x, h, g = M.build(c)
    T = M.case_truth(i)
    print(f"case {i}: kink margin {T.margin:.2e}")
    assert T.margin >= M.MIN_MARGIN
    netg, xg, hg = _on(dev, net, x, h)
    with torch.no_grad():
        F = _apply(netg, xg, hg, c.nb_steps)
    err = U.rel_err(F.cpu().numpy(), T.F)
    print(f"case {i}: F rel_err {err:.2e}  kernel {_kname()}")
    assert F.shape == (c.B, c.K)
    assert I.path_taken() == "hip" and "multi" in _kname()
    assert err <= TOL
    for B in (1, 16, 17):                     # slices of the same inputs: one lane, one full tile, one tile and a lane
        with torch.no_grad():
            Fb = _apply(netg, xg[:B].contiguous(), hg[:B].contiguous(), c.nb_steps)
        errb = U.rel_err(Fb.cpu().numpy(), T.F[:B])
        print(f"case {i}: B={B} rel_err {errb:.2e}")
        assert Fb.shape == (B, c.K) and errb <= TOL


def test_forward_nonzero_x0_and_empty_interval(dev):
    c = M.CASES[1]
    net, x, h, g = M.build(c)
    x0 = torch.randn(c.B, 1, generator=torch.Generator().manual_seed(8))      # (seed 7 draws a float64 kink margin of 1.2e-7)
    x0[5] = x[5]                              # one row with x == x0: F = 0 exactly
    T = M.truth(net, x, h, g, c.nb_steps, x0=x0)
    assert T.margin >= M.MIN_MARGIN
    netg, xg, hg, x0g = _on(dev, net, x, h, x0)
    with torch.no_grad():
        F = _apply(netg, xg, hg, c.nb_steps, x0=x0g)
    err = U.rel_err(F.cpu().numpy(), T.F)
    print(f"x0 != 0: rel_err {err:.2e}")
    assert err <= TOL and I.path_taken() == "hip"
    assert torch.equal(F[5], torch.zeros_like(F[5]))


def test_forward_integrand_network_sigmoid(dev):
    torch.manual_seed(1)
    net = IntegrandNetwork(nnets=1, nin=3, hidden_sizes=[20, 33, 17], nout=5, act_func="Sigmoid")
    _, x, h, g = M.build(M.CASES[1])
    assert mlp_spec(net) is not None and mlp_spec(net).linears[-1].out_features == 5
    F64 = M.quadrature64(copy.deepcopy(net).double(), torch.zeros_like(x).double(), x.double(), h.double(), 20).detach().numpy()
    netg = copy.deepcopy(net).to(dev)
    with torch.no_grad():
        F = _apply(netg, x.to(dev), h.to(dev), 20)
    err = U.rel_err(F.cpu().numpy(), F64)
    print(f"IntegrandNetwork/Sigmoid: rel_err {err:.2e}")
    assert err <= TOL and I.path_taken() == "hip" and "multi" in _kname()


def test_forward_inv_f(dev):
    c = M.CASES[0]
    net, x, h, g = M.build(c)
    T = M.case_truth(0, True)
    netg, xg, hg = _on(dev, net, x, h)
    with torch.no_grad():
        F = _apply(netg, xg, hg, c.nb_steps, inv_f=True)
    err = U.rel_err(F.cpu().numpy(), T.F)
    print(f"inv_f: rel_err {err:.2e}")
    assert err <= TOL and I.path_taken() == "hip"


# ------------------------------------------------------------------------------------------------------------ columns
def _row_spec(spec, k):
    last = spec.linears[-1]
    return MlpSpec(spec.linears[:-1] + [TensorLinear(last.weight[k:k + 1], last.bias[k:k + 1])], spec.hidden_act, spec.out_act)


@pytest.mark.parametrize("i", [0, 1, 2, 3])
def test_columns_equal_single_output_kernel(dev, i):
    """Column k = the existing single-output fp32 kernel on last-layer row k (catches any mix-up of k = 4r + g), and the multi
    path gives the same bits under every precision setting."""
    c = M.CASES[i]
    net, x, h, g = M.build(c)
    netg, xg, hg = _on(dev, net, x, h)
    spec = mlp_spec(netg)
    umnn_amd.set_forward_precision("fp32")
    with torch.no_grad():
        cols = torch.cat([I.hip_forward(_row_spec(spec, k), None, xg, hg, c.nb_steps)[0] for k in range(c.K)], 1)
    assert "multi" not in _kname()
    first = None
    for fwd, bwd in PRECISIONS:
        umnn_amd.set_forward_precision(fwd)
        umnn_amd.set_backward_precision(bwd)
        with torch.no_grad():
            F = _apply(netg, xg, hg, c.nb_steps)
        assert "multi" in _kname()
        err = U.rel_err(F.cpu().numpy(), cols.cpu().numpy())
        print(f"case {i} [{fwd}]: columns vs single-output fp32 {err:.2e}")
        assert err <= TOL
        first = F if first is None else first
        assert torch.equal(F, first)


# ------------------------------------------------------------------------------------------------------------ backward
def _grads(net, x, h, g, nb_steps, inv_f=False, want=("x", "h", "theta")):
    net.zero_grad()
    xr = x.clone().requires_grad_("x" in want)
    hr = h.clone().requires_grad_("h" in want)
    for p in net.parameters():
        p.requires_grad_("theta" in want)
    F = _apply(net, xr, hr, nb_steps, inv_f=inv_f)
    (F * g).sum().backward()
    torch.cuda.synchronize()
    return xr.grad, hr.grad, [p.grad for p in net.parameters()]


def _check_grads(tag, T, dx, dh, dps):
    if dx is not None:
        e = U.scaled_err(dx.cpu().numpy(), T.dx)
        print(f"{tag}: dx {e:.2e}")
        assert e <= TOL
    if dh is not None:
        e = U.scaled_err(dh.cpu().numpy(), T.dh)
        print(f"{tag}: dh {e:.2e}")
        assert e <= TOL
    if dps[0] is not None:
        for j, (p, t) in enumerate(zip(dps, T.dparams)):
            e = U.scaled_err(p.cpu().numpy(), t)
            print(f"{tag}: dparam[{j}] {tuple(t.shape)} {e:.2e}")
            assert e <= TOL


@pytest.mark.parametrize("i", [0, 1, 2, 3])
def test_backward_matches_float64(dev, i):
    c = M.CASES[i]
    net, x, h, g = M.build(c)
    T = M.case_truth(i)
    assert T.margin >= M.MIN_MARGIN
    netg, xg, hg, gg = _on(dev, net, x, h, g)
    dx, dh, dps = _grads(netg, xg, hg, gg, c.nb_steps)
    assert I.backward_path_taken() == "hip"
    assert "multi" in _lib.lib().umnn_last_kernel_name_of(_lib.PROF_BACKWARD).decode()
    _check_grads(f"case {i}", T, dx, dh, dps)
    dx2, dh2, dps2 = _grads(netg, xg, hg, gg, c.nb_steps)          # no float atomics: bit-identical
    assert torch.equal(dx, dx2) and torch.equal(dh, dh2) and all(torch.equal(a, b) for a, b in zip(dps, dps2))


def test_backward_inv_f(dev):
    c = M.CASES[1]
    net, x, h, g = M.build(c)
    T = M.case_truth(1, True)
    netg, xg, hg, gg = _on(dev, net, x, h, g)
    dx, dh, dps = _grads(netg, xg, hg, gg, c.nb_steps, inv_f=True)
    assert I.backward_path_taken() == "hip"
    _check_grads("inv_f", T, dx, dh, dps)


@pytest.mark.parametrize("want", [("h",), ("theta",)])
def test_backward_subsets(dev, want):
    c = M.CASES[2]
    net, x, h, g = M.build(c)
    T = M.case_truth(2)
    netg, xg, hg, gg = _on(dev, net, x, h, g)
    dx, dh, dps = _grads(netg, xg, hg, gg, c.nb_steps, want=want)
    assert I.backward_path_taken() == "hip"
    assert dx is None and (dh is None) == ("h" not in want) and (dps[0] is None) == ("theta" not in want)
    _check_grads(f"only {want[0]}", T, dx, dh, dps)


# ------------------------------------------------------------------------------------------------------------ n_out = 17
def test_seventeen_outputs_run_on_aten(dev):
    c = M.CASES[4]
    net, x, h, g = M.build(c)
    T = M.case_truth(4)
    assert T.margin >= M.MIN_MARGIN
    from umnn_amd import nets
    nets._noticed.discard("wide")
    netg, xg, hg, gg = _on(dev, net, x, h, g)
    with warnings.catch_warnings(record=True) as rec:
        warnings.simplefilter("always")
        with torch.no_grad():
            F = _apply(netg, xg, hg, c.nb_steps)
        assert I.path_taken() == "aten"
        dx, dh, dps = _grads(netg, xg, hg, gg, c.nb_steps)
    assert I.backward_path_taken() == "aten"
    assert len([w for w in rec if "n_out = 17" in str(w.message)]) == 1
    err = U.rel_err(F.cpu().numpy(), T.F)
    print(f"case 4: F rel_err {err:.2e}")
    assert F.shape == (c.B, 17) and err <= TOL
    _check_grads("case 4", T, dx, dh, dps)


# ------------------------------------------------------------------------------------------------------------ MonotonicNN
def _mono_pair(dev, n_out=4, nb_steps=20, B=64):
    torch.manual_seed(3)
    m = umnn_amd.MonotonicNN(3, [100, 100, 100], nb_steps=nb_steps, n_out=n_out)
    gen = torch.Generator().manual_seed(11)
    x = torch.randn(B, 1, generator=gen) * 2
    h = torch.randn(B, 2, generator=gen)
    y = torch.randn(B, n_out, generator=gen)
    return m, x, h, y


def _mono64(m64, x, h):
    """forward of a float64 copy with the plain-torch quadrature (autograd through the nodes)."""
    out = m64.net(h)
    K = m64.n_out
    F = M.quadrature64(m64.integrand, torch.zeros_like(x), x, h, m64.nb_steps)
    return torch.exp(out[:, K:]) * F + out[:, :K]


def test_monotonic_adam_step_matches_float64(dev):
    m, x, h, y = _mono_pair(dev)
    m64 = copy.deepcopy(m).double()
    mg = copy.deepcopy(m).to(dev)
    opt64 = torch.optim.Adam(m64.parameters(), lr=1e-3)
    optg = torch.optim.Adam(mg.parameters(), lr=1e-3)
    loss64 = ((_mono64(m64, x.double(), h.double()) - y.double()) ** 2).mean()
    loss64.backward()
    opt64.step()
    out = mg(x.to(dev), h.to(dev))
    assert out.shape == (64, 4) and I.path_taken() == "hip" and "multi" in _kname()
    loss = ((out - y.to(dev)) ** 2).mean()
    loss.backward()
    optg.step()
    assert I.backward_path_taken() == "hip"
    e = abs(loss.item() - loss64.item()) / max(abs(loss64.item()), 1.0)
    print(f"loss {loss.item():.6f} vs {loss64.item():.6f}: {e:.2e}")
    assert e <= TOL
    # one Adam step moves every parameter by ~lr whatever the size of its gradient: compared on the scale of the tensor
    for (name, p), p64 in zip(mg.named_parameters(), m64.parameters()):
        e = U.scaled_err(p.detach().cpu().numpy(), p64.detach().numpy())
        print(f"{name}: {e:.2e}")
        assert e <= TOL, name


def test_monotonic_inverse_round_trip(dev):
    m, x, h, _ = _mono_pair(dev)
    mg = copy.deepcopy(m).to(dev)
    xg, hg = x.to(dev), h.to(dev)
    with torch.no_grad():
        y = mg(xg, hg)
        xi, fx, status = mg.inverse(y[:, [2]].contiguous(), hg, output=2, return_info=True)
        assert I.path_taken() == "hip"
        back = mg(xi, hg)[:, 2]
    assert int((status.cpu() & (umnn_amd.SOLVE_CAPPED | umnn_amd.SOLVE_NONFINITE)).max()) == 0
    e = U.rel_err(back.cpu().numpy(), y[:, 2].cpu().numpy())
    print(f"inverse round trip: {e:.2e}")
    assert e <= 1e-4          # the solve's own tolerance (1e-6 on t) times the forward parity of the single-output kernels


# ------------------------------------------------------------------------------------------------------------ graph mode
def _compile_run(mg, xg, hg, yg, fn):
    mg.zero_grad()
    xr = xg.clone().requires_grad_()
    hr = hg.clone().requires_grad_()
    out = fn(xr, hr)
    ((out - yg) ** 2).sum().backward()
    return [out.detach(), xr.grad, hr.grad] + [p.grad.clone() for p in mg.parameters()]


def test_compile_fullgraph_is_bit_identical(dev):
    """The recorded graph keeps the HIP kernels and computes eager's bits: asserted on ``backend="aot_eager"``, which runs the graph's
    ops as they are (the single-output test of tests/test_gpu_torch_compile.py does the same; the default backend: next test)."""
    import torch._dynamo
    m, x, h, y = _mono_pair(dev, nb_steps=10, B=33)
    mg = copy.deepcopy(m).to(dev)
    xg, hg, yg = x.to(dev), h.to(dev), y.to(dev)
    eager = _compile_run(mg, xg, hg, yg, mg)
    torch._dynamo.reset()
    compiled = _compile_run(mg, xg, hg, yg, torch.compile(mg, fullgraph=True, backend="aot_eager"))
    torch._dynamo.reset()
    assert "multi" in _kname() and I.backward_path_taken() == "hip"
    for a, b in zip(eager, compiled):
        assert a.shape == b.shape and torch.equal(a, b)


def test_compile_inductor_keeps_the_kernels(dev):
    """``torch.compile(m, fullgraph=True)`` with the default Inductor backend: the conditioner's glue around the op (``scaling *
    integral + offset`` and its backward) is code Inductor generates -- it contracts the multiply-add, eager does not, and the output
    differs from eager in the last bit (measured: worst scaled error 1.5e-7) -- so the bound here is the 1e-5 of this module, on the
    scale of each tensor, not bit identity."""
    pytest.importorskip("triton")
    import torch._dynamo
    m, x, h, y = _mono_pair(dev, nb_steps=10, B=33)
    mg = copy.deepcopy(m).to(dev)
    xg, hg, yg = x.to(dev), h.to(dev), y.to(dev)
    eager = _compile_run(mg, xg, hg, yg, mg)
    torch._dynamo.reset()
    inductor = _compile_run(mg, xg, hg, yg, torch.compile(mg, fullgraph=True))
    torch._dynamo.reset()
    assert "multi" in _kname() and I.backward_path_taken() == "hip"
    worst = max(U.scaled_err(b.cpu().numpy(), a.cpu().numpy()) for a, b in zip(eager, inductor))
    print(f"inductor vs eager: worst scaled error {worst:.2e}")
    assert worst <= TOL


def test_export_keeps_the_multi_op(dev):
    m, x, h, _ = _mono_pair(dev, nb_steps=10, B=33)
    mg = copy.deepcopy(m).to(dev).eval()
    xg, hg = x.to(dev), h.to(dev)
    ep = torch.export.export(mg, (xg, hg))
    assert "umnn.cc_forward_multi" in str(ep.graph)
    with torch.no_grad():
        assert torch.equal(ep.module()(xg, hg), mg(xg, hg))


# ------------------------------------------------------------------------------------------------------------ C ABI, d = 3
def test_abi_with_three_dimensions(dev):
    B, d, E, K, n = 5, 3, 2, 5, 20
    torch.manual_seed(5)
    net = M.IntegrandNN([1 + E, 20, 33, 17, K], "LeakyReLU")
    gen = torch.Generator().manual_seed(105)
    x = torch.randn(B, d, generator=gen) * 2
    h = torch.randn(B, E * d, generator=gen)                       # [B, E*d]: index e*d + i
    g = torch.randn(B, d, K, generator=gen)
    # truth: the B*d integrals as rows [x_bi, h_b0i, h_b1i]
    rows_x = x.reshape(B * d, 1)
    rows_h = h.view(B, E, d).transpose(1, 2).reshape(B * d, E)
    T = M.truth(net, rows_x, rows_h, g.reshape(B * d, K), n)
    assert T.margin >= M.MIN_MARGIN
    netg = copy.deepcopy(net).to(dev)
    spec = mlp_spec(netg)
    desc, keep = I._desc(spec)
    lib = _lib.lib()
    xg, hg, gg = x.to(dev), h.to(dev), g.to(dev).contiguous()
    w, s = I.device_tables(n, dev)
    F, fx, fx0 = (torch.empty(B, d, K, device=dev) for _ in range(3))
    p = I._ptr
    rc = lib.umnn_cc_forward_multi(ctypes.byref(desc), None, p(xg), p(hg), p(w), p(s), n, B, d, E, 0, p(F), p(fx), p(fx0), None)
    assert rc == 0, lib.umnn_last_error()
    torch.cuda.synchronize()
    e = U.rel_err(F.cpu().numpy().reshape(B * d, K), T.F)
    print(f"ABI d=3: F {e:.2e}")
    assert e <= TOL and "multi" in _kname()
    nbytes = lib.umnn_cc_backward_multi_workspace_bytes(ctypes.byref(desc), B, d, E)
    assert nbytes > 0
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    n_params = sum(q.numel() for q in netg.parameters())
    dx, dh, dth = torch.empty(B, d, device=dev), torch.empty(B, E * d, device=dev), torch.empty(n_params, device=dev)
    rc = lib.umnn_cc_backward_multi(ctypes.byref(desc), None, p(xg), p(hg), p(gg), p(w), p(s), n, B, d, E, 0,
                                    None, p(dx), p(dh), p(dth), p(ws), nbytes, None)
    assert rc == 0, lib.umnn_last_error()
    torch.cuda.synchronize()
    dh_rows = dh.cpu().view(B, E, d).transpose(1, 2).reshape(B * d, E).numpy()
    flat64 = np.concatenate([t.reshape(-1) for t in T.dparams])
    errs = (U.scaled_err(dx.cpu().numpy().reshape(B * d, 1), T.dx), U.scaled_err(dh_rows, T.dh),
            max(U.scaled_err(a.cpu().numpy(), t) for a, t in zip(I.split_flat(dth, [q.shape for q in netg.parameters()],
                                                                            [True] * 8), T.dparams)))
    print("ABI d=3: dx %.2e dh %.2e dtheta %.2e" % errs)
    assert max(errs) <= TOL and flat64.size == n_params


def test_empty_batch(dev):
    c = M.CASES[0]
    net, x, h, g = M.build(c)
    netg = copy.deepcopy(net).to(dev)
    n0 = _lib.lib().umnn_launch_count()
    xe = torch.empty(0, 1, device=dev, requires_grad=True)
    he = torch.empty(0, 2, device=dev)
    F = _apply(netg, xe, he, c.nb_steps)
    assert F.shape == (0, c.K)
    F.sum().backward()
    assert xe.grad.shape == (0, 1)
    assert _lib.lib().umnn_launch_count() == n0
