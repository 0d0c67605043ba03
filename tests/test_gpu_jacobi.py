"""The all-dimension Newton solve (umnn_cc_solve_block) and ``invert(method="jacobi")`` on the device.

Truth and bounds are those of tests/test_gpu_inverse.py / tests/test_gpu_solve_coverage.py: the float64 oracle, TOL = 1e-4 the forward
parity tolerance, |x_hat - x| <= TOL / min(scale f) over the rows under test, residual <= TOL max(1, |t|) in the float64 oracle,
rel_err(f_x, f(x_hat)) < TOL.  Inputs: default-initialised IntegrandNetwork(d, 1 + E, hid, 1), x ~ 1.5 N(0, 1), h ~ N(0, 1), distinct
log-scales per dimension, the offset taken from embedding row 0.  The small block is B = 5, d = 7: 35 rows = three tiles, the last of three
lanes, every tile straddling samples."""
import copy
import types

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


def _oracle_net(net):
    lins = [m for m in net.net if isinstance(m, torch.nn.Linear)]
    return O.Net([l.weight.detach().cpu().double().numpy() for l in lins], [l.bias.detach().cpu().double().numpy() for l in lins],
                 O.LEAKY, O.ELU1)


_CASES = {}


def _case(hid, E, B, d, n, dev, solve_truth=True):
    """One net with the operands of a block solve and its float64 truth, computed once and shared; nothing in it is modified afterwards.
    The targets are the images of x (no |x| below 0.05, none beyond 3.5); ``solve_truth``: the truth is T.solve64 over T.integral_map of
    those targets (it differs from x by the solve's own 1e-15), else x itself."""
    key = (tuple(hid), E, B, d, n)
    if key not in _CASES:
        torch.manual_seed(31 * len(hid) + hid[0] + E + d)
        net = umnn_amd.IntegrandNetwork(d, 1 + E, list(hid), 1)
        onet = _oracle_net(net)
        g = torch.Generator().manual_seed(131 * B + n + d)
        x = (torch.randn(B, d, generator=g, dtype=torch.float64) * 1.5).clamp(-3.5, 3.5)
        x = torch.where(x.abs() < 0.05, torch.full_like(x, 0.05), x)
        h = torch.randn(B, E * d, generator=g)
        s = torch.linspace(-0.4, 0.5, d) if d > 1 else torch.tensor([0.3])
        xn, hn, sn = x.numpy(), h.double().numpy(), s.double().numpy()
        scale, off = np.exp(sn)[None, :], hn.reshape(B, E, d)[:, 0, :]
        G = T.integral_map(onet, hn, n, scale=scale, off=off)
        t64 = G(xn)[0]
        x64 = T.solve64(G, t64) if solve_truth else xn
        assert np.max(np.abs(x64 - xn)) < 1e-9
        net = net.to(dev)
        _CASES[key] = types.SimpleNamespace(net=net, spec=mlp_spec(net), onet=onet, n=n, B=B, d=d, E=E, xn=x64, hn=hn, G=G, t64=t64,
                                            h=h.to(dev), s=s.to(dev), t=torch.from_numpy(t64).float().to(dev), sf64=G(x64)[1],
                                            scale=scale)
    return _CASES[key]


def _solve(c, t=None, h=None, **kw):
    """One launch through the C entry point -> (x, f_x, status), each [B, d]."""
    before = _lib.lib().umnn_launch_count()
    out = I.hip_solve_block(c.spec, c.h if h is None else h, c.t if t is None else t, c.n, scaling=c.s, off_h0=True, **kw)
    assert out is not None and umnn_amd.path_taken() == "hip"
    assert _lib.lib().umnn_launch_count() - before == 1, "an fp16-piece launch and its queued pass count as one"
    assert _kname().startswith("cc_solve_"), _kname()
    return out


def _against_truth(c, x_hat, fx, status, tag, rows=slice(None)):
    """The three truth bounds on samples ``rows`` and no flag anywhere in them."""
    xh = x_hat.cpu().numpy().astype(np.float64)
    bound = TOL / float(c.sf64[rows].min())
    err = float(np.max(np.abs(xh - c.xn)[rows]))
    g, sf = c.G(xh)
    res = float(np.max((np.abs(g - c.t64) / np.maximum(1., np.abs(c.t64)))[rows]))
    fx_err = U.rel_err(fx.cpu().numpy()[rows], (sf / c.scale)[rows])
    evals, clamped, capped, nonfinite = (f[rows] for f in _flags(status))
    print(f"{tag}: |x_hat - x| {err:.2e} = {err / bound:.3f} of the bound {bound:.2e}, residual {res:.2e}, f_x {fx_err:.2e}, "
          f"evaluations {evals.min()}..{evals.max()}")
    assert err <= bound and res <= TOL and fx_err < TOL, tag
    assert not clamped.any() and not capped.any() and not nonfinite.any() and evals.min() >= 1, tag
    return bound


# ---- 1. every solve variant family, all four arithmetic modes ------------------------------------------------------------------
NETS = [([50] * 4, 30), ([60] * 3, 4), ([100] * 4, 10), ([100, 50, 50, 50, 50], 30), ([40, 33], 3)]


@pytest.mark.parametrize("precision", MODES)
@pytest.mark.parametrize("hid,E", NETS, ids=["x".join(map(str, hid)) for hid, _ in NETS])
def test_block_solve_against_truth_and_the_per_dimension_solve(hid, E, precision, dev):
    umnn_amd.set_forward_precision(precision)
    c = _case(hid, E, 5, 7, 20, dev)
    x_hat, fx, status = _solve(c)
    name = _kname()
    bound = _against_truth(c, x_hat, fx, status, f"{name} {precision}")
    # d calls of umnn_cc_solve on the same embedding
    x_dim = torch.full((c.B, c.d), float("nan"), device=dev)
    s_dim = torch.zeros(c.B, c.d, dtype=torch.int32, device=dev)
    for j in range(c.d):
        out = I.hip_solve(c.spec, c.h, c.t, c.n, j=j, scaling=c.s, off_h0=True, x_out=x_dim)
        assert out is not None and _kname() == name, (_kname(), name)
        s_dim[:, j] = out[2]
    assert float((x_hat - x_dim).abs().max()) <= bound
    diff = _flags(status)[0].astype(np.int64) - _flags(s_dim)[0].astype(np.int64)
    print(f"evaluations, block - per dimension: [{diff.min()}, {diff.max()}]")
    assert np.abs(diff).max() <= 1


@pytest.mark.parametrize("precision", MODES)
def test_block_of_one_dimension(precision, dev):
    """d = 1: the flat index is the sample; 37 rows (a five-lane tail)."""
    umnn_amd.set_forward_precision(precision)
    c = _case([50] * 4, 30, 37, 1, 20, dev)
    x_hat, fx, status = _solve(c)
    bound = _against_truth(c, x_hat, fx, status, f"d = 1 {precision}")
    x_dim = I.hip_solve(c.spec, c.h, c.t, c.n, j=0, scaling=c.s, off_h0=True)[0]
    assert float((x_hat - x_dim).abs().max()) <= bound


# ---- 2. warm start -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", MODES)
def test_warm_start(precision, dev):
    umnn_amd.set_forward_precision(precision)
    c = _case([50] * 4, 30, 5, 7, 20, dev)
    x1, fx1, s1 = _solve(c)
    assert _flags(s1)[0].min() >= 2
    # started on the previous output: one evaluation per row, the same bits
    x2, fx2, s2 = _solve(c, x_init=x1)
    assert torch.equal(s2, torch.ones_like(s2)) and torch.equal(x2, x1) and torch.equal(fx2, fx1)
    # x_init may be x itself
    buf = x1.clone()
    x3, fx3, s3 = _solve(c, x_init=buf, x_out=buf)
    assert x3 is buf and torch.equal(s3, torch.ones_like(s3)) and torch.equal(buf, x1) and torch.equal(fx3, fx1)
    # a start value outside [lo, hi] is clamped: after one evaluation the start point is what leaves
    for start, end in ((80., 6.), (-80., -4.)):
        x4, _, s4 = _solve(c, x_init=torch.full_like(x1, start), lo=-4., hi=6., max_iter=1)
        assert torch.all(x4 == end) and np.all(_flags(s4)[0] == 1)
    # a non-finite entry is a cold start for that row: the bits and the count of the cold launch; every other row one evaluation
    init = x1.clone()
    cold = torch.zeros(c.B, c.d, dtype=torch.bool, device=dev)
    cold[0, 2], cold[2, 1], cold[4, 6], cold[3, 0] = True, True, True, True
    init[cold] = float("nan")
    init[3, 0] = float("inf")
    x5, fx5, s5 = _solve(c, x_init=init)
    assert torch.equal(x5, x1) and torch.equal(fx5, fx1)
    assert torch.equal(s5[cold], s1[cold]) and torch.equal(s5[~cold], torch.ones_like(s5[~cold]))
    # near the solution: fewer evaluations than cold, inside the bound
    x6, fx6, s6 = _solve(c, x_init=x1 + 1e-3)
    _against_truth(c, x6, fx6, s6, f"warm start {precision}")
    assert _flags(s6)[0].max() <= 2


# ---- 3. both launch plans ------------------------------------------------------------------------------------------------------
def _unsplit_samples(wpb, d):
    """Samples of d = 3 dimensions whose B d rows the split plan refuses on this device: more than 8 CUs / wpb tiles (twice that many,
    as _unsplit_batch of tests/test_gpu_solve_coverage.py), ending in a five-row tail tile."""
    assert d == 3
    rows = 2 * 16 * (8 * torch.cuda.get_device_properties(0).multi_processor_count // wpb) + 5
    B = (rows + d - 1) // d
    while (B * d) % 16 != 5:
        B += 1
    return B


@pytest.mark.parametrize("precision", ["f16x3", "bf16x3"])
def test_both_launch_plans(precision, dev):
    """One tile per wave on the large block (every row against the truth, the tail tile on its own as well); its first 16 samples
    alone are three tiles, which the split plan takes: the same solutions within the bound."""
    umnn_amd.set_forward_precision(precision)
    d = 3
    c = _case([50] * 4, 30, _unsplit_samples(4, d), d, 20, dev, solve_truth=False)
    assert (c.B * d) % 16 == 5
    x_big, fx_big, s_big = _solve(c)
    _against_truth(c, x_big, fx_big, s_big, f"one tile per wave, {c.B} x {d} rows {precision}")
    _against_truth(c, x_big, fx_big, s_big, f"tail tile {precision}", rows=slice(c.B - 2, c.B))
    nb = 16
    x_small, fx_small, s_small = _solve(c, t=c.t[:nb].contiguous(), h=c.h[:nb].contiguous())
    bound = TOL / float(c.sf64[:nb].min())
    assert float((x_small - x_big[:nb]).abs().max()) <= bound
    assert float(np.max(np.abs(x_small.cpu().numpy() - c.xn[:nb]))) <= bound
    assert not any(f.any() for f in _flags(s_small)[1:])
    print(f"split and unsplit plan differ in some bit: {not (torch.equal(x_small, x_big[:nb]) and torch.equal(fx_small, fx_big[:nb]))}")


# ---- 4. flags and protocols ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", MODES)
def test_flags(precision, dev):
    umnn_amd.set_forward_precision(precision)
    c = _case([50] * 4, 30, 5, 7, 20, dev)
    x_ref, fx_ref, s_ref = _solve(c)
    # targets beyond G(lo) / G(hi): the endpoint, CLAMPED; every other row unflagged and inside the bound
    lo, hi = -4., 6.
    up, down = [(0, 1), (2, 6), (4, 6)], [(1, 0), (3, 3), (4, 4)]
    g_hi, g_lo = c.G(np.full_like(c.xn, hi))[0], c.G(np.full_like(c.xn, lo))[0]
    t = c.t.clone()
    for b, i in up:
        t[b, i] = float(g_hi[b, i]) + 1.
    for b, i in down:
        t[b, i] = float(g_lo[b, i]) - 1.
    x_hat, fx, status = _solve(c, t=t, lo=lo, hi=hi)
    evals, clamped, capped, nonfinite = _flags(status)
    ends = np.zeros((c.B, c.d), bool)
    for b, i in up:
        ends[b, i] = True
        assert float(x_hat[b, i]) == hi and clamped[b, i]
    for b, i in down:
        ends[b, i] = True
        assert float(x_hat[b, i]) == lo and clamped[b, i]
    assert not clamped[~ends].any() and not capped.any() and not nonfinite.any()
    assert float(np.max(np.abs(x_hat.cpu().numpy() - c.xn)[~ends])) <= TOL / float(c.sf64.min())
    # a NaN target or a NaN embedding entry: NaN + NONFINITE for that (b, i) only, every other row the bits of the clean launch
    t, h = c.t.clone(), c.h.clone()
    bad = torch.zeros(c.B, c.d, dtype=torch.bool, device=dev)
    t[0, 3], t[4, 5] = float("nan"), float("nan")
    h.view(c.B, c.E, c.d)[2, 7, 1] = float("nan")
    bad[0, 3], bad[4, 5], bad[2, 1] = True, True, True
    x_hat, fx, status = _solve(c, t=t, h=h)
    evals, clamped, capped, nonfinite = _flags(status)
    nb = bad.cpu().numpy()
    assert torch.isnan(x_hat[bad]).all() and nonfinite[nb].all() and not nonfinite[~nb].any() and not capped.any() and not clamped.any()
    assert torch.equal(x_hat[~bad], x_ref[~bad]) and torch.equal(fx[~bad], fx_ref[~bad]) and torch.equal(status[~bad], s_ref[~bad])
    # max_iter = 1: the start point, one evaluation, CAPPED (no target is within tol of G(0): |x| >= 0.05)
    x_hat, fx, status = _solve(c, max_iter=1)
    evals, clamped, capped, nonfinite = _flags(status)
    assert torch.all(x_hat == 0.) and np.all(evals == 1) and capped.all() and not clamped.any() and not nonfinite.any()
    f0 = c.G(np.zeros_like(c.xn))[1] / c.scale
    assert U.rel_err(fx.cpu().numpy(), f0) < TOL


def test_overflowing_rows_are_redone_on_bf16_pieces(dev):
    """tests/test_gpu_solve_coverage.py::test_overflowing_rows_on_the_unsplit_plan for the block solve: the embedding of three (b, i)
    pairs -- one of them in the three-lane tail tile -- times 3e6 overflows the fp16 pieces.  Those rows hold the bf16x3 mode's numbers
    bit for bit, every other row -- their tile mates included -- the numbers of the fp16-piece launch without an overflowing row; the
    pair of launches counts as one (_solve).  Warm-started with x_init aliasing x, the deferred rows restart cold in the queued pass."""
    c = _case([50] * 4, 30, 5, 7, 20, dev)
    hot = torch.zeros(c.B, c.d, dtype=torch.bool, device=dev)
    hot[0, 3], hot[2, 0], hot[4, 6] = True, True, True
    h = c.h.clone()
    h3 = h.view(c.B, c.E, c.d)
    for b, i in hot.nonzero().tolist():
        h3[b, :, i] *= 3e6
    t = torch.randn(c.B, c.d, generator=torch.Generator().manual_seed(2)).to(dev)
    umnn_amd.set_forward_precision("bf16x3")
    xb, fb, sb = _solve(c, t=t, h=h)
    assert _kname().startswith("cc_solve_bf16<")
    umnn_amd.set_forward_precision("f16x3")
    xf, ff, sf = _solve(c, t=t, h=h)
    assert _kname().startswith("cc_solve_f16<")
    xs, fs, ss = _solve(c, t=t)                                   # (the same launch with no overflowing row)
    assert torch.isfinite(xf).all() and torch.isfinite(ff).all()
    assert torch.equal(xf[hot], xb[hot]) and torch.equal(ff[hot], fb[hot]) and torch.equal(sf[hot], sb[hot])
    assert torch.equal(xf[~hot], xs[~hot]) and torch.equal(ff[~hot], fs[~hot]) and torch.equal(sf[~hot], ss[~hot])
    assert not _flags(sf)[2].any() and not _flags(sf)[3].any()
    # the embedding really overflows fp16 pieces: the forward defers the tile groups of these rows too (equal to bf16x3)
    umnn_amd.set_forward_precision("bf16x3")
    Fb = I.hip_forward(c.spec, None, xf, h, c.n)[0]
    umnn_amd.set_forward_precision("f16x3")
    Ff = I.hip_forward(c.spec, None, xf, h, c.n)[0]
    assert torch.equal(Ff[hot], Fb[hot])
    # warm start through the aliased buffer: a deferred row has lost its start value to the NaN marker and restarts cold
    buf = xs.clone()
    xw, fw, sw = _solve(c, t=t, h=h, x_init=buf, x_out=buf)
    assert torch.equal(xw[hot], xb[hot]) and torch.equal(sw[hot], sb[hot])
    assert torch.equal(xw[~hot], xs[~hot]) and torch.equal(sw[~hot], torch.ones_like(sw[~hot]))


# ---- 5. the flow ---------------------------------------------------------------------------------------------------------------
def _flow_bound(m, x, context):
    """sum over blocks of TOL / min exp(s) f, from the model's own log_jac pieces in float64 on the CPU."""
    m64 = copy.deepcopy(m).to("cpu").double()
    umnn_amd.invalidate_caches(m64)
    xi = x.detach().cpu().double()
    ctx = None if context is None else context.detach().cpu().double()
    total = 0.
    with torch.no_grad():
        for blk in m64.nets:
            z, lj = blk._transform(xi, ctx, want_jac=True)
            total += TOL / float(torch.exp(lj.min()))
            xi = torch.flip(z, [1])
    return total


def _flow(d, hid, E, n, nb_flow, dev, seed, cond_in=0, made_gain=1.):
    torch.manual_seed(seed)
    m = umnn_amd.UMNNMAFFlow(nb_flow=nb_flow, nb_in=d, hidden_derivative=list(hid), hidden_embedding=[64, 64], embedding_s=E,
                             nb_steps=n, solver="CCParallel", cond_in=cond_in).to(dev).eval()
    if made_gain != 1.:
        with torch.no_grad():
            for blk in m.nets:
                for mod in blk.net.made.net:
                    if hasattr(mod, "weight"):
                        mod.weight.mul_(made_gain)
        umnn_amd.invalidate_caches(m)
    return m


def _round_trip(m, x, ctx, d, tag, **kw):
    """x -> z -> invert(method="jacobi"): the flow bound, m(x_hat) = z, the HIP path, one solve launch per sweep, sweeps <= d."""
    bound = _flow_bound(m, x, ctx)
    with torch.no_grad():
        z = m(x, context=ctx)
        before = _lib.lib().umnn_launch_count()
        x_hat, info = m.invert(z, method="jacobi", context=ctx, return_info=True, **kw)
        launches = _lib.lib().umnn_launch_count() - before
        assert umnn_amd.path_taken() == "hip" and _kname().startswith("cc_solve_"), _kname()
        z_back = m(x_hat, context=ctx)
    err = float((x_hat - x).abs().max())
    print(f"{tag}: |x_hat - x| {err:.2e} (bound {bound:.2e}), sweeps {info['sweeps']}, evaluations per sweep {info['max_evals']}")
    assert launches == sum(info["sweeps"]), (launches, info["sweeps"])
    assert all(1 <= s <= d for s in info["sweeps"]) and all(info["converged"])
    assert all(not f.any() for st in info["status"] for f in _flags(st)[1:])
    assert err <= bound
    assert U.rel_err(z_back.cpu().numpy(), z.cpu().numpy()) < TOL
    return x_hat, info, z, bound


FLOWS = [(7, [50] * 4, 30, 50, 2, 33), (2, [100] * 4, 10, 50, 1, 64), (5, [100, 50, 50, 50, 50], 8, 30, 1, 20), (3, [40, 33], 4, 20, 2, 17)]


@pytest.mark.parametrize("precision", MODES)
@pytest.mark.parametrize("d,hid,E,n,nb_flow,B", FLOWS, ids=[f"d{f[0]}-{'x'.join(map(str, f[1]))}" for f in FLOWS])
def test_flow_round_trip(d, hid, E, n, nb_flow, B, precision, dev):
    umnn_amd.set_forward_precision(precision)
    m = _flow(d, hid, E, n, nb_flow, dev, seed=d + E)
    x = 1.5 * torch.randn(B, d, generator=torch.Generator().manual_seed(B)).to(dev)
    _round_trip(m, x, None, d, f"jacobi d={d} {hid} {precision}")


def test_flow_with_stronger_coupling(dev):
    """MADE weights x 3: more sweeps, still at most d, and the sequential method's answer within the bound."""
    d = 7
    m = _flow(d, [50] * 4, 30, 50, 2, dev, seed=3, made_gain=3.)
    x = 1.5 * torch.randn(33, d, generator=torch.Generator().manual_seed(1)).to(dev)
    x_hat, info, z, bound = _round_trip(m, x, None, d, "jacobi, MADE weights x 3")
    assert max(info["sweeps"]) > 2
    with torch.no_grad():
        x_seq = m.invert(z, method="newton")
        x_all, info_all = m.invert(z, method="jacobi", sweep_tol=0., return_info=True)
        x_one, info_one = m.invert(z, method="jacobi", max_sweeps=1, return_info=True)
    assert float((x_hat - x_seq).abs().max()) <= bound
    assert info_all["sweeps"] == [d, d] and float((x_all - x_seq).abs().max()) <= bound
    assert info_one["sweeps"] == [1, 1] and info_one["converged"] == [False, False]


def test_conditional_flow_with_context(dev):
    d, cond, B = 3, 3, 33
    m = _flow(d, [50] * 4, 30, 20, 2, dev, seed=23, cond_in=cond, made_gain=3.)
    g = torch.Generator().manual_seed(6)
    x = (1.5 * torch.randn(B, d, generator=g)).to(dev)
    ctx = torch.randn(B, cond, generator=g).to(dev)
    x_hat, info, z, bound = _round_trip(m, x, ctx, d, "jacobi, conditional flow")
    with torch.no_grad():
        x_other = m.invert(z, method="jacobi", context=torch.flip(ctx, [0]))
    assert float((x_other - x).abs().max()) > 100 * bound, "the context is really read"


def test_jacobi_with_bf16_embedding_matches_fp32_embedding(dev):
    """tests/test_gpu_solve_coverage.py::test_newton_with_bf16_embedding_matches_fp32_embedding for method="jacobi": the embedding is
    widened to fp32 for the solve; samples agree with the fp32-embedding ones to the embedding's rounding and round-trip."""
    d = 6
    m = _flow(d, [50] * 3, 8, 30, 2, dev, seed=5)
    z = torch.randn(200, d, generator=torch.Generator().manual_seed(0)).to(dev)
    with torch.no_grad():
        x32 = m.invert(z, method="jacobi")
        m.set_embedding_dtype(torch.bfloat16)
        try:
            before = _lib.lib().umnn_launch_count()
            x16, info = m.invert(z, method="jacobi", return_info=True)
            assert _lib.lib().umnn_launch_count() - before == sum(info["sweeps"]) and _kname().startswith("cc_solve_"), _kname()
            assert umnn_amd.path_taken() == "hip" and m.nets[0].net.m_embeding.dtype == torch.bfloat16
            z_back = m.forward(x16)
        finally:
            m.set_embedding_dtype(None)
    assert all(s <= d for s in info["sweeps"])
    assert torch.isfinite(x16).all() and not torch.equal(x16, x32)
    assert float((x16 - x32).abs().max()) < 5e-2 * max(1.0, float(x32.abs().max()))
    assert float((z_back - z).abs().max()) < 5e-2 * max(1.0, float(z.abs().max()))
