"""The inverse direction without a GPU: ``MonotonicNN.inverse``, ``InverseNeuralIntegral`` and ``invert(method="newton")`` on
the generic ATen path against a float64 truth solve (tests/_inverse_truth.py), their gradients, and the ``umnn::cc_solve`` op's
schema, fake shapes and refusals.

Bounds.  A forward value that is off by the project's forward parity tolerance TOL = 1e-4 (tests/test_gpu_forward.py) moves the
solution of G(x) = y by TOL / G'(x), so |x_hat - x| is held to TOL / min G' with G' = exp(s) f(x) taken from the float64 oracle on
the rows under test -- for a flow, summed over its blocks.  The residual is held to TOL * max(1, |y|) in the float64 oracle."""
import subprocess
import sys

import numpy as np
import pytest
import torch
from torch._subclasses.fake_tensor import FakeTensorMode
from torch.fx.experimental.symbolic_shapes import DimDynamic, ShapeEnv, StatelessSymbolicContext

import umnn_amd
from oracle import cc_oracle as O
from tests import _inverse_truth as T
from tests import _util as U
from umnn_amd import integral
from umnn_amd.nets import IntegrandNetwork

TOL = 1e-4          # forward parity tolerance of the project (tests/test_gpu_forward.py)
MAX_EVALS = 8       # the reference arithmetic needs <= 5 on these cases; room for rounding, none for a broken step rule


def _monotonic(n, dtype=torch.float32):
    G = U.load(f"g5_monotonic_n{n}")
    m = umnn_amd.MonotonicNN(3, [100, 100, 100], nb_steps=n, dev="cpu")
    m.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in U.state_dict_of(G).items()})
    return G, m.to(dtype)


def _status(status):
    s = status.numpy()
    return s & umnn_amd.SOLVE_EVALS_MASK, (s & umnn_amd.SOLVE_CLAMPED) != 0, (s & umnn_amd.SOLVE_CAPPED) != 0


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
@pytest.mark.parametrize("n", [50, 100])
def test_monotonic_inverse_recovers_fixture_x(n, dtype):
    G, m = _monotonic(n, dtype)
    net, cW, cb = T.monotonic_parts(G)
    G64 = T.monotonic_map(net, cW, cb, G["h"], n)
    y64, dy = G64(G["x"].astype(np.float64))
    bound = TOL / float(dy.min())
    assert 1e-5 < bound < 1e-3, bound                                  # min exp(s) f is of order one: the bound is not vacuous
    y, h = torch.from_numpy(G["y"]).to(dtype), torch.from_numpy(G["h"]).to(dtype)
    with torch.no_grad():
        x_hat, fx, status = m.inverse(y, h, return_info=True)
    assert umnn_amd.path_taken() == "aten"
    assert x_hat.shape == y.shape and x_hat.dtype == dtype and fx.shape == y.shape and status.dtype == torch.int32
    err = float(np.max(np.abs(x_hat.numpy().astype(np.float64) - G["x"])))
    res = np.abs(G64(x_hat.numpy().astype(np.float64))[0] - G["y"]) / np.maximum(1., np.abs(G["y"]))
    evals, clamped, capped = _status(status)
    print(f"n={n} {dtype}: |x_hat - x| {err:.2e} (bound {bound:.2e}), residual {res.max():.2e}, evaluations <= {evals.max()}")
    assert err <= bound
    assert res.max() <= TOL
    assert not clamped.any() and not capped.any()
    assert evals.max() <= MAX_EVALS and evals.min() >= 1
    # f(x) is the integrand at the solution: dy/dx = exp(s) f
    assert U.rel_err(fx.numpy(), O.integrand(net, x_hat.numpy().astype(np.float64), G["h"].astype(np.float64))) < 1e-5
    # ... and against the truth solve of the fixture's y
    x_true = T.solve64(G64, G["y"])
    assert np.max(np.abs(x_hat.numpy() - x_true)) <= bound


@pytest.mark.parametrize("n", [50, 100])
def test_monotonic_inverse_on_a_wide_range(n):
    G, m = _monotonic(n)
    rng = np.random.default_rng(5)
    x = rng.uniform(-8., 8., size=G["x"].shape).astype(np.float32)
    net, cW, cb = T.monotonic_parts(G)
    G64 = T.monotonic_map(net, cW, cb, G["h"], n)
    y64, dy = G64(x.astype(np.float64))
    bound = TOL / float(dy.min())
    with torch.no_grad():
        x_hat, _, status = m.inverse(torch.from_numpy(y64.astype(np.float32)), torch.from_numpy(G["h"]), return_info=True)
    evals, clamped, capped = _status(status)
    assert np.max(np.abs(x_hat.numpy() - x)) <= bound
    assert not clamped.any() and not capped.any() and evals.max() <= MAX_EVALS


def test_targets_outside_the_range_end_on_the_endpoint():
    G, m = _monotonic(50)
    net, cW, cb = T.monotonic_parts(G)
    h = G["h"][:8]
    G64 = T.monotonic_map(net, cW, cb, h, 50)
    hi, lo = G64(np.full((8, 1), 50.))[0], G64(np.full((8, 1), -50.))[0]
    inside = G64(np.full((8, 1), 0.5))[0]
    ht = torch.from_numpy(h)
    with torch.no_grad():
        for y, end in ((hi + 1., 50.), (lo - 1., -50.)):
            x_hat, _, status = m.inverse(torch.from_numpy(y.astype(np.float32)), ht, return_info=True)
            evals, clamped, capped = _status(status)
            assert np.all(x_hat.numpy() == end) and clamped.all() and not capped.any() and evals.max() <= MAX_EVALS
        # a narrower range clamps accordingly; rows whose target is inside it are not flagged
        y = np.concatenate([G64(np.full((8, 1), 3.))[0][:4], inside[4:]])
        x_hat, _, status = m.inverse(torch.from_numpy(y.astype(np.float32)), ht, x_range=(-1., 1.), return_info=True)
        evals, clamped, capped = _status(status)
        assert np.all(x_hat.numpy()[:4] == 1.) and clamped[:4].all()
        assert np.max(np.abs(x_hat.numpy()[4:] - 0.5)) < 1e-4 and not clamped[4:].any() and not capped.any()
        x_hat = m.inverse(torch.from_numpy(G64(np.full((8, 1), -3.))[0].astype(np.float32)), ht, x_range=(-1., 1.))
        assert np.all(x_hat.numpy() == -1.)


def test_infinite_targets_end_on_the_endpoint():
    """tol * max(1, |y|) is infinite for an infinite y: the residual test must not take that for convergence at the start point."""
    G, m = _monotonic(50)
    y = torch.from_numpy(G["y"][:8]).clone()
    y[1], y[6] = float("inf"), float("-inf")
    with torch.no_grad():
        for lo, hi in ((-50., 50.), (0.5, 8.)):
            x_hat, _, status = m.inverse(y, torch.from_numpy(G["h"][:8]), x_range=(lo, hi), return_info=True)
            evals, clamped, capped = _status(status)
            assert float(x_hat[1]) == hi and float(x_hat[6]) == lo and clamped[1] and clamped[6] and not capped.any()
            assert evals.max() <= MAX_EVALS and torch.isfinite(x_hat).all()


def test_max_iter_caps_and_flags():
    G, m = _monotonic(50)
    with torch.no_grad():
        _, _, status = m.inverse(torch.from_numpy(G["y"]), torch.from_numpy(G["h"]), max_iter=1, return_info=True)
    evals, _, capped = _status(status)
    assert capped.any() and evals.max() == 1


# ---- gradients ------------------------------------------------------------------------------------------------------------
# Convention.  The implicit backward divides by f(x), the derivative of the EXACT integral -- the library's (and the reference's)
# Leibniz convention for limits, oracle.cc_oracle.integrate_backward -- while finite differences of a solve see the derivative of
# the discrete quadrature, dF_n/dx.  Per row the two gradients therefore differ by the factor f / (dF_n/dx) = 1 + delta exactly,
# with delta the quadrature's own derivative error (spectrally small for a smooth integrand, ~1e-3 for a ReLU net at n = 50).
class _SmoothIntegrand(torch.nn.Module):
    """A small net with smooth activations (mlp_spec does not recognise it: the generic path): delta ~ 1e-10 at n = 40."""

    def __init__(self, E):
        super().__init__()
        self.l1, self.l2 = torch.nn.Linear(1 + E, 8), torch.nn.Linear(8, 1)

    def forward(self, x, h):
        return torch.nn.functional.softplus(self.l2(torch.tanh(self.l1(torch.cat((x, h), 1))))) + 0.2


def test_gradcheck_of_inverse_neural_integral():
    E, B, n = 3, 5, 40
    torch.manual_seed(0)
    net = _SmoothIntegrand(E).double()
    params = list(net.parameters())
    theta0 = integral._flatten(params).detach()

    def fn(t, h, theta):
        with torch.no_grad():          # the integrand reads its own parameters: hand it the perturbed ones
            o = 0
            for p in params:
                p.copy_(theta[o:o + p.numel()].view(p.shape))
                o += p.numel()
        return umnn_amd.InverseNeuralIntegral.apply(t, net, theta, h, n, (-50., 50.), 1e-14, 64)

    g = torch.Generator().manual_seed(1)
    t = (torch.randn(B, 1, generator=g, dtype=torch.float64) * 1.5).requires_grad_()
    h = torch.randn(B, E, generator=g, dtype=torch.float64).requires_grad_()
    theta = theta0.clone().requires_grad_()
    assert torch.autograd.gradcheck(fn, (t, h, theta), eps=1e-6, atol=1e-7, rtol=1e-6, nondet_tol=0.0)
    # the forward solves what it says: int_0^x f = t
    x = fn(t, h, theta0).detach()
    assert umnn_amd.path_taken() == "aten"
    F = umnn_amd.ParallelNeuralIntegral.apply(torch.zeros_like(x), x, net, theta0, h.detach(), n)
    assert float((F - t.detach()).abs().max()) < 1e-12


def test_inverse_neural_integral_backward_is_the_implicit_formula():
    """MLP integrand (LeakyReLU: kinks) with d > 1, against the oracle: g_t = g / f(x), (d_theta, d_h) = integrate_backward's for
    the upper limit x and the cotangent -g / f(x)."""
    d, E, B, n = 2, 3, 7, 30
    torch.manual_seed(0)
    net = IntegrandNetwork(d, 1 + E, [12, 12], 1).double()
    g = torch.Generator().manual_seed(1)
    t = (torch.randn(B, d, generator=g, dtype=torch.float64) * 1.5).requires_grad_()
    h = torch.randn(B, E * d, generator=g, dtype=torch.float64).requires_grad_()
    theta = integral._flatten(net.parameters())
    cot = torch.randn(B, d, generator=g, dtype=torch.float64)
    x = umnn_amd.InverseNeuralIntegral.apply(t, net, theta, h, n, (-50., 50.), 1e-14)
    gt, gh, *gp = torch.autograd.grad(x, [t, h] + list(net.parameters()), cot)
    lins = [m for m in net.net if isinstance(m, torch.nn.Linear)]
    onet = O.Net([l.weight.detach().numpy() for l in lins], [l.bias.detach().numpy() for l in lins], O.LEAKY, O.ELU1)
    xn, hn = x.detach().numpy(), h.detach().numpy()
    # (the package's quadrature tables are stored in fp32 -- 6e-8 relative -- also when the tensors are float64)
    assert np.max(np.abs(O.integrate_parallel(onet, np.zeros_like(xn), xn, hn, n) - t.detach().numpy())) < 1e-6
    f = O.integrand(onet, xn, hn)
    _, _, dh, _, _, flat = O.integrate_backward(onet, np.zeros_like(xn), xn, hn, n, -cot.numpy() / f)
    assert U.scaled_err(gt.numpy(), cot.numpy() / f) < 1e-6
    assert U.scaled_err(gh.numpy(), dh) < 1e-6
    assert U.scaled_err(integral._flatten(gp).numpy(), flat) < 1e-6


def test_monotonic_inverse_gradients_match_central_differences_of_the_truth():
    """Gradients of one row's x w.r.t. y, h and all parameters against float64 central differences of the truth solve, each within
    that row's |delta| (see above; measured here with the oracle) of the analytic value."""
    n = 50
    G, m = _monotonic(n, torch.float64)
    sd0 = {k: v.detach().numpy().copy() for k, v in m.state_dict().items()}
    eps = 1e-6
    rng = np.random.default_rng(0)

    def parts(sd):
        iW, ib, _ = U._seq(sd, "integrand.net.", np.float64)
        cW, cb, _ = U._seq(sd, "net.", np.float64)
        return O.Net(iW, ib, O.RELU, O.ELU1), cW, cb

    for row in (0, 3, 11):
        y0, h0 = G["y"][[row]].astype(np.float64), G["h"][[row]].astype(np.float64)
        y, h = torch.from_numpy(y0).requires_grad_(), torch.from_numpy(h0).requires_grad_()
        m.zero_grad()
        x = m.inverse(y, h, tol=1e-14)
        x.sum().backward()
        net, cW, cb = parts(sd0)
        x64 = T.solve64(T.monotonic_map(net, cW, cb, h0, n), y0)
        assert abs(x.item() - x64.item()) < 1e-6
        Fp = O.integrate_parallel(net, np.zeros_like(x64), x64 + eps, h0, n)
        Fm = O.integrate_parallel(net, np.zeros_like(x64), x64 - eps, h0, n)
        delta = abs(O.integrand(net, x64, h0).item() / ((Fp - Fm) / (2 * eps)).item() - 1.)
        assert delta < 1e-2, delta

        def central(perturb):
            vals = []
            for sgn in (+1., -1.):
                sd = {k: v.copy() for k, v in sd0.items()}
                yv, hv = y0.copy(), h0.copy()
                perturb(sd, yv, hv, sgn * eps)
                vals.append(T.solve64(T.monotonic_map(*parts(sd), hv, n), yv).item())
            return (vals[0] - vals[1]) / (2 * eps)

        def close(fd, an, what):
            assert abs(fd - an) <= 1.5 * delta * abs(an) + 1e-7, (row, what, fd, an, delta)

        close(central(lambda sd, yv, hv, e: yv.__setitem__((0, 0), yv[0, 0] + e)), float(y.grad), "y")
        for c in range(h0.shape[1]):
            close(central(lambda sd, yv, hv, e, c=c: hv.__setitem__((0, c), hv[0, c] + e)), float(h.grad[0, c]), ("h", c))
        # every parameter tensor: its largest-gradient entry and two random ones
        for k, p in m.named_parameters():
            gflat = p.grad.reshape(-1).numpy()
            for ii in {int(np.argmax(np.abs(gflat)))} | {int(v) for v in rng.integers(0, gflat.size, 2)}:
                def pert(sd, yv, hv, e, k=k, ii=ii):
                    sd[k].reshape(-1)[ii] += e
                close(central(pert), float(gflat[ii]), (k, ii))


# ---- flow -------------------------------------------------------------------------------------------------------------------
def _g6():
    G = U.load("g6_invert")
    m = umnn_amd.UMNNMAFFlow(nb_flow=2, nb_in=2, hidden_derivative=[50] * 3, hidden_embedding=[32, 32],
                             embedding_s=10, nb_steps=30, solver="CCParallel")
    m.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in U.state_dict_of(G).items()})
    m.eval()
    return G, m


def test_flow_newton_inversion_against_the_fixture_and_the_truth():
    G, m = _g6()
    blocks = T.blocks_from_state_dict(U.state_dict_of(G), 2)
    mins = T.flow_min_sf(blocks, G["x"], 30)
    bound = sum(TOL / v for v in mins)
    assert 1e-4 < bound < 1e-3, (mins, bound)
    z = torch.from_numpy(G["z"])
    with torch.no_grad():
        x_hat = m.invert(z, method="newton")
        x_blk = m.invert(z, iter=3, method="newton", tol=1e-6, max_iter=64)        # iter is ignored
    assert torch.equal(x_hat, x_blk)
    err = float(np.max(np.abs(x_hat.numpy() - G["x"])))
    print(f"flow newton: |x_hat - x| {err:.2e} (bound {bound:.2e})")
    assert err <= bound
    assert float(np.max(np.abs(x_hat.numpy() - G["x_inv"]))) < 2 * 100. / 9 ** 5       # the fixture's own resolution
    x_true, _ = T.flow_invert64(blocks, G["z"], 30)
    assert float(np.max(np.abs(x_hat.numpy() - x_true))) <= bound
    # a single block as well
    with torch.no_grad():
        z1 = m.nets[0](torch.from_numpy(G["x"]))
        x1 = m.nets[0].invert(z1, method="newton")
    assert float(np.max(np.abs(x1.numpy() - G["x"]))) <= TOL / mins[0]


def test_flow_newton_on_random_rows():
    G, m = _g6()
    blocks = T.blocks_from_state_dict(U.state_dict_of(G), 2)
    x = (1.5 * np.random.default_rng(3).standard_normal((64, 2))).astype(np.float32)
    bound = sum(TOL / v for v in T.flow_min_sf(blocks, x, 30))
    z = O.flow_forward(blocks, x.astype(np.float64), 30).astype(np.float32)
    with torch.no_grad():
        x_hat = m.invert(torch.from_numpy(z), method="newton")
    assert float(np.max(np.abs(x_hat.numpy() - x))) <= bound


def test_default_method_is_the_untouched_bracket_search():
    G, m = _g6()
    z = torch.from_numpy(G["z"])
    with torch.no_grad():
        ref = umnn_amd.sampling.run(list(m.nets), True, z, None, umnn_amd.sampling.Options(iter=5)).x
        assert torch.equal(m.invert(z, iter=5), ref)
        assert torch.equal(m.invert(z, 5, None), ref)
        assert torch.equal(m.invert(z, iter=5, method="bracket"), ref)
        blk = m.nets[1]
        assert torch.equal(blk.invert(z, iter=4), umnn_amd.sampling.invert_bracket(blk, z, None, umnn_amd.sampling.Options(iter=4)).x)
    with pytest.raises(ValueError, match="unknown inversion method"):
        m.invert(z, method="secant")
    with pytest.raises(ValueError, match="unknown inversion method"):
        m.nets[0].invert(z, method="secant")


# ---- the op ---------------------------------------------------------------------------------------------------------------
def _net(E, hidden, device="cuda"):
    sizes = [1 + E] + list(hidden) + [1]
    return ([torch.empty(o, i, device=device) for i, o in zip(sizes, sizes[1:])], [torch.empty(o, device=device) for o in sizes[1:]])


def test_cc_solve_is_registered_with_its_schema():
    assert "cc_solve" in umnn_amd.ops.OPS
    schema = torch.ops.umnn.cc_solve.default._schema
    assert [a.name for a in schema.arguments] == ["t", "h", "W", "b", "hidden_act", "out_act", "nb_steps", "lo", "hi", "tol", "max_iter"]
    assert len(schema.returns) == 3
    assert not any(a.alias_info is not None and a.alias_info.is_write for a in schema.arguments)


@pytest.mark.parametrize("B,d,E", [(1, 1, 2), (65536, 1, 2), (100, 3, 30)])
def test_cc_solve_fake_shapes(B, d, E):
    with FakeTensorMode():
        t, h = torch.empty(B, d, device="cuda", requires_grad=True), torch.empty(B, E * d, device="cuda")
        W, b = _net(E, [50, 50, 50])
        W = [w.requires_grad_() for w in W]
        x, fx, status = torch.ops.umnn.cc_solve(t, h, W, b, 1, 0, 50, -50., 50., 1e-6, 64)
        assert x.shape == fx.shape == status.shape == (B, d)
        assert x.dtype == fx.dtype == torch.float32 and status.dtype == torch.int32 and x.device.type == "cuda"
        assert x.requires_grad and not fx.requires_grad and not status.requires_grad


def test_cc_solve_fake_shapes_with_a_symbolic_batch():
    mode = FakeTensorMode(shape_env=ShapeEnv())
    ctx = StatelessSymbolicContext(dynamic_sizes=[DimDynamic.DYNAMIC, DimDynamic.STATIC])
    E = 2
    t = mode.from_tensor(torch.empty(256, 1, device="meta"), symbolic_context=ctx)
    h = mode.from_tensor(torch.empty(256, E, device="meta"), symbolic_context=ctx)
    with mode:
        t, h = t.to("cuda"), h.to("cuda")
        W, b = _net(E, [100, 100, 100])
        B = t.shape[0]
        assert isinstance(B, torch.SymInt)
        x, fx, status = torch.ops.umnn.cc_solve(t, h, W, b, 1, 0, 50, -50., 50., 1e-6, 64)
    for o in (x, fx, status):
        assert o.shape[0] == B and o.shape[1] == 1


def test_cc_solve_refuses_what_the_kernels_cannot_take():
    with FakeTensorMode():
        B, d, E, n = 16, 3, 4, 10
        t, h = torch.empty(B, d, device="cuda"), torch.empty(B, E * d, device="cuda")
        W, b = _net(E, [20, 20])
        u = torch.ops.umnn
        cases = [
            (lambda: u.cc_solve(t.cpu(), h.cpu(), [w.cpu() for w in W], [v.cpu() for v in b], 0, 0, n, -50., 50., 1e-6, 64), "x is on cpu"),
            (lambda: u.cc_solve(t, h, [w.cpu() for w in W], b, 0, 0, n, -50., 50., 1e-6, 64), r"cc_solve: W\[0\] is on cpu"),
            (lambda: u.cc_solve(t.double(), h, W, b, 0, 0, n, -50., 50., 1e-6, 64), "cc_solve: x has dtype torch.float64"),
            (lambda: u.cc_solve(t, h[:, :-1], W, b, 0, 0, n, -50., 50., 1e-6, 64), "cc_solve: h has shape"),
            (lambda: u.cc_solve(t[0], h, W, b, 0, 0, n, -50., 50., 1e-6, 64), "cc_solve: x has shape"),
            (lambda: u.cc_solve(t, h, [w.double() for w in W], b, 0, 0, n, -50., 50., 1e-6, 64), "integrand weights must be fp32"),
            (lambda: u.cc_solve(t, h, W, b, 0, 0, n, 1., 1., 1e-6, 64), "empty bracket"),
            (lambda: u.cc_solve(t, h, W, b, 0, 0, n, -50., 50., 1e-6, 0), "max_iter is 0"),
            (lambda: u.cc_solve(t, h, W, b, 0, 0, 0, -50., 50., 1e-6, 64), "nb_steps is 0"),
        ]
        for call, msg in cases:
            with pytest.raises(RuntimeError, match=msg):
                call()


def test_import_still_loads_no_library():
    code = ("import sys, torch, umnn_amd\n"
            "from umnn_amd import _lib\n"
            "assert _lib._lib is None, 'libumnn_cc loaded at import'\n"
            "assert hasattr(torch.ops.umnn, 'cc_solve') and 'cc_solve' in umnn_amd.ops.OPS\n"
            "assert callable(umnn_amd.MonotonicNN.inverse) and umnn_amd.InverseNeuralIntegral is not None\n"
            "maps = open('/proc/self/maps').read() if sys.platform.startswith('linux') else ''\n"
            "assert 'libumnn_cc' not in maps\n"
            "assert not torch.cuda.is_initialized()\n"
            "assert 'torch._dynamo' not in sys.modules, 'import umnn_amd pulled in torch._dynamo'\n"
            "print('ok')\n")
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and out.stdout.strip().endswith("ok"), out.stderr


def test_solve_entry_point_validates_without_a_gpu():
    import ctypes
    from umnn_amd import _lib
    lib = _lib.lib()
    p = ctypes.c_void_p(0x1000)
    d = _lib.MlpDesc()
    d.n_linear = 3
    for i, w in enumerate([3, 16, 16, 1]):
        d.widths[i] = w
    for l in range(3):
        d.W[l], d.b[l] = 0x1000, 0x1000

    def call(B=4, j=0, lo=-50., hi=50., max_iter=64, nb_steps=20, x=p):
        return lib.umnn_cc_solve(ctypes.byref(d), p, p, 1, None, None, None, 0, p, p, nb_steps, B, 1, 2, j, lo, hi, 1e-6, max_iter,
                                 x, 1, None, None, None)
    assert call(B=0) == 0                                 # an empty batch is a no-op and touches no device
    assert call(j=1) == _lib.EINVAL and call(lo=1., hi=1.) == _lib.EINVAL and call(max_iter=0) == _lib.EINVAL
    assert call(nb_steps=0) == _lib.EINVAL and call(x=None) == _lib.EINVAL
