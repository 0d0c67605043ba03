"""The in-kernel Newton solve (umnn_cc_solve) on the GPU: against a float64 truth solve in every forward arithmetic mode, against
the host-driven loop, through UMNNMAFFlow.invert(method="newton"), the small-batch split plan, the fp16 overflow protocol, the
gradients of MonotonicNN.inverse and torch.compile / torch.export.

Bounds (as in tests/test_inverse_cpu.py): |x_hat - x| <= TOL / min G' with TOL = 1e-4 the forward parity tolerance and
G' = exp(s) f(x) from float64 arithmetic on the rows under test, summed over the blocks of a flow; residual <= TOL max(1, |y|)."""
import copy
import warnings

import numpy as np
import pytest
import torch

import umnn_amd
from oracle import cc_oracle as O
from tests import _inverse_truth as T
from tests import _util as U
from umnn_amd import _lib, integral as I
from umnn_amd.nets import mlp_spec

pytestmark = pytest.mark.gpu
TOL = 1e-4
MODES = ["f16x3", "bf16x3", "bf16x6", "fp32"]


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


def _flags(status):
    s = status.cpu().numpy()
    return (s & umnn_amd.SOLVE_EVALS_MASK, (s & umnn_amd.SOLVE_CLAMPED) != 0, (s & umnn_amd.SOLVE_CAPPED) != 0,
            (s & umnn_amd.SOLVE_NONFINITE) != 0)


def _expect_kernel(name, precision, wide):
    """The solve's arithmetic follows cc_invert's tables: fp16 pieces by default and for wide nets under "exact products",
    three bf16 pieces for nets of up to four tiles per layer under bf16x6 / fp32."""
    on_f16 = precision == "f16x3" or (precision in ("bf16x6", "fp32") and wide)
    assert name.startswith("cc_solve_f16<" if on_f16 else "cc_solve_bf16<"), name
    assert ("PARTS=3" in name) == (precision in ("bf16x6", "fp32") and not wide), name


def _oracle_net(net, hidden_act=O.LEAKY):
    lins = [m for m in net.net if isinstance(m, torch.nn.Linear)]
    return O.Net([l.weight.detach().cpu().double().numpy() for l in lins], [l.bias.detach().cpu().double().numpy() for l in lins],
                 hidden_act, O.ELU1)


# ---- 1. kernel vs float64 truth, every arithmetic mode -------------------------------------------------------------------------
@pytest.mark.parametrize("precision", MODES)
@pytest.mark.parametrize("n", [50, 100])
def test_monotonic_inverse_matches_the_truth(n, precision, dev):
    umnn_amd.set_forward_precision(precision)
    G = U.load(f"g5_monotonic_n{n}")
    m = umnn_amd.MonotonicNN(3, [100, 100, 100], nb_steps=n, dev=dev)
    m.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in U.state_dict_of(G).items()})
    m.to(dev)
    net, cW, cb = T.monotonic_parts(G)
    G64 = T.monotonic_map(net, cW, cb, G["h"], n)
    bound = TOL / float(G64(G["x"].astype(np.float64))[1].min())
    before = _lib.lib().umnn_launch_count()
    with torch.no_grad():
        x_hat, fx, status = m.inverse(torch.from_numpy(G["y"]).to(dev), torch.from_numpy(G["h"]).to(dev), return_info=True)
    assert umnn_amd.path_taken() == "hip" and _lib.lib().umnn_launch_count() - before == 1
    _expect_kernel(_kname(), precision, wide=True)
    assert "T=7" in _kname(), _kname()
    xh = x_hat.cpu().numpy().astype(np.float64)
    err = float(np.max(np.abs(xh - G["x"])))
    res = float(np.max(np.abs(G64(xh)[0] - G["y"]) / np.maximum(1., np.abs(G["y"]))))
    evals, clamped, capped, nonfinite = _flags(status)
    print(f"g5 n={n} {precision}: |x_hat - x| {err:.2e} (bound {bound:.2e}), residual {res:.2e}, evaluations <= {evals.max()}")
    assert err <= bound and res <= TOL
    assert not clamped.any() and not capped.any() and not nonfinite.any() and evals.min() >= 1
    assert U.rel_err(fx.cpu().numpy(), O.integrand(net, xh, G["h"].astype(np.float64))) < TOL


NETS = {"flow_50x4": ([50] * 4, 30, 100), "wide_first": ([100, 50, 50, 50, 50], 30, 100), "ragged": ([40, 33], 4, 20)}


@pytest.mark.parametrize("precision", MODES)
@pytest.mark.parametrize("net_name", sorted(NETS))
def test_kernel_matches_the_truth(net_name, precision, dev):
    """InverseNeuralIntegral on the kernel for batches that are and are not multiples of the 16-row tile."""
    umnn_amd.set_forward_precision(precision)
    hid, E, n = NETS[net_name]
    torch.manual_seed(len(hid) * 31 + E)
    net = umnn_amd.IntegrandNetwork(1, 1 + E, hid, 1).to(dev)
    onet = _oracle_net(net)
    spec = mlp_spec(net)
    for B in (1, 17, 100, 8192):
        g = torch.Generator().manual_seed(B)
        x = torch.randn(B, 1, generator=g, dtype=torch.float64) * 1.5
        h = torch.randn(B, E, generator=g)
        xn, hn = x.numpy(), h.double().numpy()
        t64 = O.integrate_parallel(onet, np.zeros_like(xn), xn, hn, n)
        bound = TOL / float(O.integrand(onet, xn, hn).min())
        before = _lib.lib().umnn_launch_count()
        x_hat, fx, status = I.solve_integral(spec, torch.from_numpy(t64).float().to(dev), h.to(dev), n, -50., 50., 1e-6, 64)
        assert umnn_amd.path_taken() == "hip" and _lib.lib().umnn_launch_count() - before == 1
        name = _kname()
        _expect_kernel(name, precision, wide=max(hid) > 63)
        if net_name == "flow_50x4":
            assert "T=4" in name and "LIVE=13" in name, name
        if net_name == "wide_first":
            assert "T1=7,TREST=4" in name, name
        xh = x_hat.cpu().numpy().astype(np.float64)
        err = float(np.max(np.abs(xh - xn)))
        res = float(np.max(np.abs(O.integrate_parallel(onet, np.zeros_like(xh), xh, hn, n) - t64) / np.maximum(1., np.abs(t64))))
        evals, clamped, capped, nonfinite = _flags(status)
        print(f"{net_name} B={B} {precision}: |x_hat - x| {err:.2e} (bound {bound:.2e}), residual {res:.2e}, evaluations <= {evals.max()}")
        assert err <= bound and res <= TOL
        assert not clamped.any() and not capped.any() and not nonfinite.any() and evals.min() >= 1
        assert U.rel_err(fx.cpu().numpy(), O.integrand(onet, xh, hn)) < TOL


def test_targets_outside_the_range_and_strided_operands(dev):
    """The C entry point as the flow calls it: column j of [B, d] targets and outputs, exp(scaling[j]), embedding row 0 as the offset;
    targets beyond G(+-50) end on the endpoint with the clamped flag."""
    torch.manual_seed(3)
    B, d, E, n, j = 50, 3, 8, 30, 1
    net = umnn_amd.IntegrandNetwork(d, 1 + E, [50] * 4, 1).to(dev)
    onet = _oracle_net(net)
    spec = mlp_spec(net)
    h = torch.randn(B, E * d, device=dev)
    scaling = torch.tensor([0.1, -0.3, 0.2], device=dev)
    x_true = np.random.default_rng(0).uniform(-4., 4., (B, d))
    hn = h.cpu().double().numpy()
    z64 = np.exp(scaling.cpu().double().numpy())[None, :] * (O.integrate_parallel(onet, np.zeros_like(x_true), x_true, hn, n)
                                                              + hn.reshape(B, E, d)[:, 0, :])
    z64[:5, j] = 1e4
    z64[5:10, j] = -1e4
    z = torch.from_numpy(z64).float().to(dev)
    x_out = torch.full((B, d), 7.0, device=dev)
    out = I.hip_solve(spec, h, z, n, j=j, scaling=scaling, off_h0=True, x_out=x_out)
    assert out is not None and out[0] is x_out
    _, fx, status = out
    evals, clamped, capped, _ = _flags(status)
    xo = x_out.cpu().numpy()
    assert np.all(xo[:, [0, 2]] == 7.0), "only column j is written"
    assert np.all(xo[:5, j] == 50.) and np.all(xo[5:10, j] == -50.) and clamped[:10].all() and not clamped[10:].any()
    assert not capped.any() and evals.max() <= 8
    bound = TOL / float((np.exp(scaling.cpu().double().numpy())[None, :] * O.integrand(onet, x_true, hn))[10:, j].min())
    assert np.max(np.abs(xo[10:, j] - x_true[10:, j])) <= bound


# ---- 2. kernel vs the host-driven loop -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("hid,E,n", [([50] * 4, 30, 100), ([100] * 3, 2, 50)])
def test_kernel_agrees_with_the_host_driven_newton(hid, E, n, dev):
    torch.manual_seed(11)
    B = 100
    net = umnn_amd.IntegrandNetwork(1, 1 + E, hid, 1).to(dev)
    onet = _oracle_net(net)
    spec = mlp_spec(net)
    x = torch.randn(B, 1, dtype=torch.float64) * 1.5
    h = torch.randn(B, E)
    t64 = O.integrate_parallel(onet, np.zeros((B, 1)), x.numpy(), h.double().numpy(), n)
    bound = TOL / float(O.integrand(onet, x.numpy(), h.double().numpy()).min())
    t, hg = torch.from_numpy(t64).float().to(dev), h.to(dev)
    xk, fk, sk = I.solve_integral(spec, t, hg, n, -50., 50., 1e-6, 64)
    assert _kname().startswith("cc_solve_")
    xh, fh, sh = I.host_solve(spec, hg, t, n, -50., 50., 1e-6, 64)
    assert not _kname().startswith("cc_solve_"), _kname()          # (the forward kernels, one launch per iteration)
    assert float((xk - xh).abs().max()) <= bound
    ek, eh = _flags(sk)[0], _flags(sh)[0]
    print(f"evaluations kernel <= {ek.max()}, host <= {eh.max()}, max difference {np.abs(ek - eh).max()}")
    assert np.abs(ek.astype(int) - eh.astype(int)).max() <= 1
    assert not _flags(sk)[2].any() and not _flags(sh)[2].any()


# ---- 3 / 4. the flow: launch count, round trip, against the bracket search -----------------------------------------------------
def _flow_bound(m, x):
    """sum over blocks of TOL / min exp(s) f, from the model's own log_jac pieces in float64 on the CPU."""
    m64 = copy.deepcopy(m).to("cpu").double()
    umnn_amd.invalidate_caches(m64)
    xi = x.detach().cpu().double()
    total = 0.
    with torch.no_grad():
        for i, blk in enumerate(m64.nets):
            z, lj = blk._transform(xi, None, want_jac=True)
            total += TOL / float(torch.exp(lj.min()))
            xi = torch.flip(z, [1])
    return total


@pytest.mark.parametrize("precision", MODES)
@pytest.mark.parametrize("d,hid,E,n,nb_flow,B", [(7, [50] * 4, 30, 50, 2, 33), (2, [100] * 4, 10, 50, 1, 64),
                                                 (5, [100, 50, 50, 50, 50], 8, 30, 1, 20), (3, [40, 33], 4, 20, 2, 17)])
def test_newton_round_trip(d, hid, E, n, nb_flow, B, precision, dev):
    umnn_amd.set_forward_precision(precision)
    torch.manual_seed(d * 7 + len(hid))
    m = umnn_amd.UMNNMAFFlow(nb_flow=nb_flow, nb_in=d, hidden_derivative=hid, hidden_embedding=[64, 64], embedding_s=E,
                             nb_steps=n, solver="CCParallel").to(dev).eval()
    x = torch.randn(B, d, device=dev) * 1.5
    bound = _flow_bound(m, x)
    with torch.no_grad():
        z = m(x)
        before = _lib.lib().umnn_launch_count()
        x_newton = m.invert(z, method="newton")
        assert _lib.lib().umnn_launch_count() - before == nb_flow * d, "exactly one solve launch per dimension and block"
        assert umnn_amd.path_taken() == "hip"
        _expect_kernel(_kname(), precision, wide=max(hid) > 63)
        with warnings.catch_warnings():
            warnings.simplefilter("ignore", RuntimeWarning)
            x_bracket = m.invert(z, iter=10)
        z2 = m(x_newton)
    e_newton, e_bracket = float((x_newton - x).abs().max()), float((x_bracket - x).abs().max())
    print(f"d={d} {hid} {precision}: newton {e_newton:.2e}, bracket(iter=10) {e_bracket:.2e}, bound {bound:.2e}")
    assert e_newton <= bound and e_bracket <= bound
    assert U.rel_err(z2.cpu().numpy(), z.cpu().numpy()) < TOL


# ---- 5. the small-batch split plan ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hid,E,n", [([100] * 4, 10, 50), ([100, 50, 50, 50, 50], 30, 100)])
def test_small_batch_split_plan_equals_the_unsplit_one(hid, E, n, dev):
    """The split plan (one tile per workgroup, its node range split over the workgroup's waves) is taken while tiles x waves per
    workgroup <= 8 per CU -- up to 8192 rows at four waves on 256 CUs --, so the B = 1 and B = 6 batches here run it; the same rows at
    the head of a batch too large for that plan run one tile per wave.  Same numbers up to the summation order.  (Every row of such
    a batch against the truth: tests/test_gpu_solve_coverage.py.)"""
    torch.manual_seed(5)
    net = umnn_amd.IntegrandNetwork(1, 1 + E, hid, 1).to(dev)
    onet = _oracle_net(net)
    spec = mlp_spec(net)
    big = 16 * 2048 + 5                      # more tiles x waves than the split plan accepts on any device (8 per CU)
    x = torch.randn(big, 1, dtype=torch.float64) * 1.5
    h = torch.randn(big, E)
    hn = h[:6].double().numpy()
    bound = TOL / float(O.integrand(onet, x[:6].numpy(), hn).min())
    with torch.no_grad():
        t = I.hip_forward(spec, None, x.float().to(dev), h.to(dev), n)[0]
    x_big, _, s_big = I.solve_integral(spec, t, h.to(dev), n, -50., 50., 1e-6, 64)
    for B in (1, 6):
        x_small, _, s_small = I.solve_integral(spec, t[:B].contiguous(), h[:B].to(dev).contiguous(), n, -50., 50., 1e-6, 64)
        assert float((x_small - x_big[:B]).abs().max()) <= bound
        assert float((x_small.cpu().double() - x[:B]).abs().max()) <= bound
        assert not _flags(s_small)[2].any()
    assert not _flags(s_big)[2].any()


# ---- 6. overflow protocol ------------------------------------------------------------------------------------------------------
def test_overflowing_rows_are_redone_on_bf16_pieces(dev):
    """Rows 0..11 carry an embedding scaled until the first hidden layer leaves fp16's range: a numerical overflow inside a healthy
    kernel.  Under the default arithmetic the result is finite; the overflowing rows hold the bf16x3 mode's numbers bit for bit and
    every other row -- those sharing a tile with them included -- the fp16-piece numbers."""
    torch.manual_seed(2)
    B, E, n = 100, 30, 50
    net = umnn_amd.IntegrandNetwork(1, 1 + E, [50] * 4, 1).to(dev)
    spec = mlp_spec(net)
    h = torch.randn(B, E, device=dev)
    h[:12] *= 3e6
    t = torch.randn(B, 1, device=dev)
    umnn_amd.set_forward_precision("bf16x3")
    xb, fb, sb = I.solve_integral(spec, t, h, n, -50., 50., 1e-6, 64)
    assert _kname().startswith("cc_solve_bf16<")
    umnn_amd.set_forward_precision("f16x3")
    before = _lib.lib().umnn_launch_count()
    xf, ff, sf = I.solve_integral(spec, t, h, n, -50., 50., 1e-6, 64)
    assert _lib.lib().umnn_launch_count() - before == 1 and _kname().startswith("cc_solve_f16<")
    assert torch.isfinite(xf).all() and torch.isfinite(ff).all()
    assert torch.equal(xf[:12], xb[:12]) and torch.equal(ff[:12], fb[:12]) and torch.equal(sf[:12], sb[:12])
    xs, fs, ss = I.solve_integral(spec, t[12:].contiguous(), h[12:].contiguous(), n, -50., 50., 1e-6, 64)
    assert torch.equal(xf[12:], xs) and torch.equal(ff[12:], fs) and torch.equal(sf[12:], ss)
    assert not torch.equal(xs, xb[12:]), "the two arithmetics differ in the last bits somewhere"
    assert not _flags(sf)[2].any() and not _flags(sf)[3].any()
    # the embedding really overflows fp16 pieces: the forward defers these rows too (NaN-free, equal to bf16x3)
    umnn_amd.set_forward_precision("bf16x3")
    Fb = I.hip_forward(spec, None, xf, h, n)[0]
    umnn_amd.set_forward_precision("f16x3")
    Ff = I.hip_forward(spec, None, xf, h, n)[0]
    assert torch.equal(Ff[:12], Fb[:12]) and not torch.equal(Ff[16:], Fb[16:])


# ---- 8. gradients --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [50, 100])
def test_monotonic_inverse_gradients_match_float64(n, dev):
    """Against the same module in float64 on the CPU (tests/test_inverse_cpu.py holds that path to the oracle's implicit formula and to
    central differences), with the tolerance tests/test_gpu_backward.py uses for this net."""
    G = U.load(f"g5_monotonic_n{n}")
    sd = {k: torch.from_numpy(np.asarray(v)) for k, v in U.state_dict_of(G).items()}
    m = umnn_amd.MonotonicNN(3, [100, 100, 100], nb_steps=n, dev=dev)
    m.load_state_dict(sd)
    m.to(dev)
    m64 = umnn_amd.MonotonicNN(3, [100, 100, 100], nb_steps=n, dev="cpu")
    m64.load_state_dict(sd)
    m64.double()
    w = torch.linspace(0.5, 1.5, G["y"].shape[0]).view(-1, 1)
    y, h = torch.from_numpy(G["y"]).to(dev).requires_grad_(), torch.from_numpy(G["h"]).to(dev).requires_grad_()
    x = m.inverse(y, h)
    assert umnn_amd.path_taken() == "hip" and _kname().startswith("cc_solve_")
    (x * w.to(dev)).sum().backward()
    assert umnn_amd.backward_path_taken() == "hip"
    y64, h64 = torch.from_numpy(G["y"]).double().requires_grad_(), torch.from_numpy(G["h"]).double().requires_grad_()
    (m64.inverse(y64, h64, tol=1e-13) * w.double()).sum().backward()
    assert U.scaled_err(y.grad.cpu().numpy(), y64.grad.numpy()) < TOL
    assert U.scaled_err(h.grad.cpu().numpy(), h64.grad.numpy()) < TOL
    for (k, p), p64 in zip(m.named_parameters(), m64.parameters()):
        assert U.scaled_err(p.grad.cpu().numpy(), p64.grad.numpy()) < TOL, k


# ---- 9. torch.compile / torch.export -------------------------------------------------------------------------------------------
def _same(a, b):
    assert a.shape == b.shape and a.dtype == b.dtype
    assert torch.equal(a, b), f"max |diff| {(a.float() - b.float()).abs().max().item()}"


class _Inverse(torch.nn.Module):
    def __init__(self, m):
        super().__init__()
        self.m = m

    def forward(self, y, h):
        return self.m.inverse(y, h)


def _inverse_grads(mod, y, h):
    mod.zero_grad()
    yg, hg = y.clone().requires_grad_(), h.clone().requires_grad_()
    x = mod(yg, hg)
    (x * torch.linspace(-1, 1, x.shape[0], device=x.device).view(-1, 1)).sum().backward()
    return [x.detach(), yg.grad, hg.grad] + [p.grad.clone() for p in mod.parameters()]


def test_opcheck_cc_solve(dev):
    torch.manual_seed(1)
    E, B = 4, 48
    net = umnn_amd.IntegrandNetwork(1, 1 + E, [32, 32], 1).to(dev)
    W, b, ha, oa = umnn_amd.ops.spec_args(mlp_spec(net))
    W, b = [w.detach() for w in W], [v.detach() for v in b]
    t, h = torch.randn(B, 1, device=dev), torch.randn(B, E, device=dev)
    torch.library.opcheck(torch.ops.umnn.cc_solve.default, (t, h, W, b, ha, oa, 16, -50., 50., 1e-6, 64))
    Wg, bg = [w.clone().requires_grad_() for w in W], [v.clone().requires_grad_() for v in b]
    torch.library.opcheck(torch.ops.umnn.cc_solve.default,
                          (t.clone().requires_grad_(), h.clone().requires_grad_(), Wg, bg, ha, oa, 16, -50., 50., 1e-6, 64))


def test_monotonic_inverse_compiles_and_exports(dev):
    import torch._dynamo
    torch._dynamo.reset()
    torch.manual_seed(0)
    m = umnn_amd.MonotonicNN(3, [100, 100, 100], nb_steps=50).to(dev)
    mod = _Inverse(m)
    y, h = torch.randn(512, 1, device=dev), torch.randn(512, 2, device=dev)
    want = _inverse_grads(mod, y, h)
    got = _inverse_grads(torch.compile(mod, backend="aot_eager", fullgraph=True), y, h)
    for a, w in zip(got, want):
        _same(a, w)
    assert umnn_amd.path_taken() == "hip" and umnn_amd.backward_path_taken() == "hip" and _kname() != ""
    batch = torch.export.Dim("batch", min=2, max=4096)
    for p in m.parameters():
        p.requires_grad_(False)
    ep = torch.export.export(mod, (y[:64], h[:64]), dynamic_shapes=({0: batch}, {0: batch}))
    assert "torch.ops.umnn.cc_solve" in ep.graph_module.print_readable(print_output=False)
    for B in (64, 300):
        with torch.no_grad():
            _same(ep.module()(y[:B], h[:B]), mod(y[:B], h[:B]))
    torch._dynamo.reset()
