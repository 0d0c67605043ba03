"""The in-kernel Newton solve (umnn_cc_solve) where tests/test_gpu_inverse.py does not reach: every row of the two variant tables
by name, both launch plans (one tile per wave / one tile per workgroup with the node range split over its waves) on every row of
the batch, the stop rules and the status word, non-finite inputs, brackets that exclude 0, the operand forms and the flow path.

Truth and bounds are those of tests/test_gpu_inverse.py: targets t64 = O.integrate_parallel(onet, 0, x, h, n) in float64,
TOL = 1e-4 the forward parity tolerance, |x_hat - x| <= TOL / min(scale f) over the rows under test, residual <= TOL max(1, |t|) in
the float64 oracle, rel_err(f_x, f(x_hat)) < TOL.  Inputs: default-initialised IntegrandNetwork(1, 1 + E, hid, 1), x ~ 1.5 N(0, 1),
h ~ N(0, 1)."""
import copy
import types
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


def _oracle_net(net, hidden_act=O.LEAKY):
    lins = [m for m in net.net if isinstance(m, torch.nn.Linear)]
    return O.Net([l.weight.detach().cpu().double().numpy() for l in lins], [l.bias.detach().cpu().double().numpy() for l in lins],
                 hidden_act, O.ELU1)


_CASES = {}


def _case(hid, E, B, n, dev, seed=0):
    """One net with its inputs and float64 truth, computed once per (net, batch, node count) and shared by every test and arithmetic
    mode that asks for it; nothing in it is modified afterwards."""
    key = (tuple(hid), E, B, n, seed)
    if key not in _CASES:
        torch.manual_seed(1000 * seed + 31 * len(hid) + hid[0] + E)
        net = umnn_amd.IntegrandNetwork(1, 1 + E, list(hid), 1)
        onet = _oracle_net(net)
        g = torch.Generator().manual_seed(7919 * seed + 131 * B + n)
        x = torch.randn(B, 1, generator=g, dtype=torch.float64) * 1.5
        h = torch.randn(B, E, generator=g)
        xn, hn = x.numpy(), h.double().numpy()
        t64 = O.integrate_parallel(onet, np.zeros_like(xn), xn, hn, n)
        net = net.to(dev)
        _CASES[key] = types.SimpleNamespace(net=net, spec=mlp_spec(net), onet=onet, n=n, B=B, E=E, xn=xn, hn=hn, h=h.to(dev), t64=t64,
                                            t=torch.from_numpy(t64).float().to(dev), f64=O.integrand(onet, xn, hn))
    return _CASES[key]


def _solve(c, lo=-50., hi=50., tol=1e-6, max_iter=64, t=None, h=None, want_info=True):
    """One launch of the kernel through the C entry point: -> (x [B,1], f_x [B], status [B])."""
    before = _lib.lib().umnn_launch_count()
    out = I.hip_solve(c.spec, c.h if h is None else h, c.t if t is None else t, c.n, lo=lo, hi=hi, tol=tol, max_iter=max_iter,
                      want_info=want_info)
    assert out is not None and umnn_amd.path_taken() == "hip" and _lib.lib().umnn_launch_count() - before == 1
    assert _kname().startswith("cc_solve_"), _kname()
    return out


def _against_truth(c, x_hat, fx, status, tag, rows=slice(None)):
    """The three truth bounds on ``rows`` of case ``c`` and no flag anywhere in them -> max |x_hat - x| / bound."""
    xh = x_hat.cpu().numpy().astype(np.float64).reshape(-1, 1)
    bound = TOL / float(c.f64[rows].min())
    err = float(np.max(np.abs(xh - c.xn)[rows]))
    res = float(np.max((np.abs(O.integrate_parallel(c.onet, np.zeros_like(xh), xh, c.hn, c.n) - c.t64) / np.maximum(1., np.abs(c.t64)))[rows]))
    evals, clamped, capped, nonfinite = (f[rows] for f in _flags(status))
    fx_err = U.rel_err(fx.cpu().numpy().reshape(-1, 1)[rows], O.integrand(c.onet, xh, c.hn)[rows])
    print(f"{tag}: |x_hat - x| {err:.2e} = {err / bound:.3f} of the bound {bound:.2e}, residual {res:.2e}, f_x {fx_err:.2e}, "
          f"evaluations {evals.min()}..{evals.max()}")
    assert err <= bound and res <= TOL and fx_err < TOL, tag
    assert not clamped.any() and not capped.any() and not nonfinite.any() and evals.min() >= 1, tag
    return err / bound


def _cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


def _unsplit_batch(wpb):
    """A batch the split plan refuses on this device: more than 8 CUs / wpb tiles (twice that many) plus a five-lane tail tile."""
    return 2 * 16 * (8 * _cus() // wpb) + 5


# ---- 1. every row of both variant tables, by name, on both launch plans ---------------------------------------------------------
# t_out = (H + 16) // 16 tiles and ks_in = (H + 4) // 4 live registers per layer of width H (umnn_prepare_mlp); a uniform net of five to
# eight tiles runs on eight waves once 2 (image bytes + 1024) exceeds 160 KiB.  (net, E, name after the build's prefix)
_TWO_PIECE = [
    ([50] * 4, 30, "<T=4,EXACT=1,LIVE=13>"),
    ([60] * 3, 4, "<T=4,EXACT=1,LIVE=0>"),
    ([40, 33], 4, "<T=4,EXACT=1,LIVE=0>"),                    # three tiles, zero-padded to four
    ([100, 100], 2, "<T=7,EXACT=1,LIVE=26>"),
    ([96, 96], 3, "<T=7,EXACT=1,LIVE=0>"),
    ([64, 64], 5, "<T=5,EXACT=1,LIVE=0>"),
    ([80, 80, 80], 6, "<T=6,EXACT=1,LIVE=0>"),
    ([112, 112], 7, "<T=8,EXACT=1,LIVE=0>"),
    ([100] * 3, 2, "<T=7,EXACT=1,LIVE=26,WAVES=8>"),
    ([96] * 3, 9, "<T=7,EXACT=1,LIVE=0,WAVES=8>"),
    ([64] * 5, 3, "<T=5,EXACT=1,LIVE=0,WAVES=8>"),
    ([80] * 4, 4, "<T=6,EXACT=1,LIVE=0,WAVES=8>"),
    ([127] * 3, 5, "<T=8,EXACT=1,LIVE=0,WAVES=8>"),
    ([20, 20], 4, "<T=2,EXACT=0,LIVE=0>"),
    ([70, 90], 4, "<T=8,EXACT=0,LIVE=0>"),
    ([64, 50, 50, 50], 8, "<T1=5,TREST=4,LIVE=13>"),
    ([80, 50, 50, 50], 8, "<T1=6,TREST=4,LIVE=13>"),
    ([100, 50, 50, 50], 8, "<T1=7,TREST=4,LIVE=13>"),
    ([127, 50, 50, 50], 8, "<T1=8,TREST=4,LIVE=13>"),
    ([79, 60, 60], 6, "<T1=5,TREST=4,LIVE=0>"),
    ([95, 63, 33], 6, "<T1=6,TREST=4,LIVE=0>"),
    ([111, 60, 60], 6, "<T1=7,TREST=4,LIVE=0>"),
    ([112, 20, 50], 6, "<T1=8,TREST=4,LIVE=0>"),
]
_THREE_PIECE = [
    ([50] * 4, 30, "<T=4,PARTS=3,EXACT=1,LIVE=13>"),
    ([60] * 3, 4, "<T=4,PARTS=3,EXACT=1,LIVE=0>"),
    ([20, 20], 4, "<T=2,PARTS=3,EXACT=0,LIVE=0>"),
]
VARIANTS = ([("f16x3", "cc_solve_f16" + name, hid, E) for hid, E, name in _TWO_PIECE]
            + [("bf16x3", "cc_solve_bf16" + name, hid, E) for hid, E, name in _TWO_PIECE]
            + [("fp32", "cc_solve_bf16" + name, hid, E) for hid, E, name in _THREE_PIECE])


@pytest.mark.parametrize("precision,name,hid,E", VARIANTS, ids=[f"{p}-{'x'.join(map(str, hid))}" for p, _, hid, _ in VARIANTS])
def test_every_table_row_by_name_on_both_plans(precision, name, hid, E, dev):
    """B = 37 rows (two full tiles and a five-lane tail) on the kernel the plan names for this net.  n = 20: three tiles are few
    enough for the split plan on any device.  n = 2: fewer nodes than waves, so the same rows run one tile per wave."""
    umnn_amd.set_forward_precision(precision)
    for n in (20, 2):
        c = _case(hid, E, 37, n, dev)
        x_hat, fx, status = _solve(c)
        assert _kname() == name, (_kname(), name)
        _against_truth(c, x_hat, fx, status, f"{name} {precision} n={n}")


def test_images_beyond_the_lds_run_the_host_loop(dev):
    """Six hidden layers of six tiles: five two-piece images are 180 KiB, beyond the 160 KiB of LDS the solve kernels accept, while
    the fp32 forward's images (157.5 KiB) fit, so the host loop has a forward to run on.  (Not 128-wide layers: 128 is nine tiles, above
    UMNN_MAX_HIDDEN_WIDTH = 127, and is refused before any image is sized; 112..127 x 4 exceeds the LDS in the forward as well.)  hip_solve declines; solve_integral finishes through the host-driven loop within the same bounds,
    infinite targets included."""
    c = _case([80] * 6, 4, 37, 20, dev)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)           # (the fallback is announced once per process)
        assert I.hip_solve(c.spec, c.h, c.t, c.n) is None
        assert "exceed 160 KiB" in _lib.lib().umnn_last_error().decode()
        x_hat, fx, status = I.solve_integral(c.spec, c.t, c.h, c.n, -50., 50., 1e-6, 64)
    assert umnn_amd.path_taken() == "hip" and not _kname().startswith("cc_solve_"), _kname()
    _against_truth(c, x_hat, fx[:, 0], status[:, 0], "host loop [80]*6")
    t = c.t.clone()
    t[1], t[2] = float("inf"), float("-inf")
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        x_inf, _, s_inf = I.solve_integral(c.spec, t, c.h, c.n, -50., 50., 1e-6, 64)
    clamped = _flags(s_inf[:, 0])[1]
    assert float(x_inf[1]) == 50. and float(x_inf[2]) == -50. and clamped[1] and clamped[2] and int(clamped.sum()) == 2
    keep = [0] + list(range(3, 37))
    assert torch.equal(x_inf[keep], x_hat[keep])


# ---- 2. both launch plans on every row of the batch ---------------------------------------------------------------------------
BIG = {"flow_50x4": ([50] * 4, 30, 4), "waves8_100x3": ([100] * 3, 2, 8), "wide_first": ([100, 50, 50, 50], 8, 4)}


@pytest.mark.parametrize("net_name,precision", [("flow_50x4", p) for p in MODES] + [("waves8_100x3", "f16x3"), ("wide_first", "f16x3")])
def test_unsplit_plan_on_every_row_of_a_large_batch(net_name, precision, dev):
    """More tiles than the split plan accepts (16 389 rows on 256 CUs at four waves per workgroup): one tile per wave.  Every row
    against the truth, the five-lane tail tile on its own as well."""
    umnn_amd.set_forward_precision(precision)
    hid, E, wpb = BIG[net_name]
    c = _case(hid, E, _unsplit_batch(wpb), 20, dev)
    x_hat, fx, status = _solve(c)
    assert ("WAVES=8" in _kname()) == (wpb == 8) and ("T1=" in _kname()) == (net_name == "wide_first"), _kname()
    ratio = _against_truth(c, x_hat, fx, status, f"unsplit {net_name} B={c.B} {precision}")
    _against_truth(c, x_hat, fx, status, f"unsplit {net_name} tail tile {precision}", rows=slice(c.B - 5, c.B))
    print(f"unsplit plan {net_name} {precision}: max |x_hat - x| / bound = {ratio:.3f}")


def test_the_two_plans_agree_and_are_two_plans(dev):
    """The first 48 rows of the large batch solved alone take the split plan: the same solutions within the bound, and -- the partial
    sums meeting in another order -- not the same bits for at least one net, the evidence that two plans ran."""
    differ = []
    for net_name, (hid, E, wpb) in BIG.items():
        c = _case(hid, E, _unsplit_batch(wpb), 20, dev)
        x_big, fx_big, s_big = _solve(c)
        x_small, fx_small, s_small = _solve(c, t=c.t[:48].contiguous(), h=c.h[:48].contiguous())
        bound = TOL / float(c.f64[:48].min())
        assert float((x_small - x_big[:48]).abs().max()) <= bound
        assert float((x_small.cpu().double() - torch.from_numpy(c.xn[:48])).abs().max()) <= bound
        assert not _flags(s_small)[2].any() and not _flags(s_small)[3].any()
        differ.append(not (torch.equal(x_small, x_big[:48]) and torch.equal(fx_small, fx_big[:48])))
        print(f"{net_name}: split and unsplit plan differ in some bit: {differ[-1]}")
    assert any(differ)


SPLIT_EDGES = [([50] * 4, 30, 4, "<T=4,EXACT=1,LIVE=13>"), ([100, 50, 50, 50], 8, 4, "<T1=7,TREST=4,LIVE=13>"),
               ([100, 100], 2, 4, "<T=7,EXACT=1,LIVE=26>"), ([100] * 3, 2, 8, "<T=7,EXACT=1,LIVE=26,WAVES=8>")]


@pytest.mark.parametrize("hid,E,wpb,name", SPLIT_EDGES, ids=[n for _, _, _, n in SPLIT_EDGES])
def test_split_plan_at_the_edges_of_the_node_partition(hid, E, wpb, name, dev):
    """Wave `part` of wpb sums nodes [part (n + 1) / wpb, (part + 1) (n + 1) / wpb): n + 1 = wpb gives every wave one node, wpb + 1 an
    uneven split, wpb + 2 another; one lane, one full tile, one tile and one lane."""
    for n in (wpb - 1, wpb, wpb + 1):
        for B in (1, 16, 17):
            c = _case(hid, E, B, n, dev)
            x_hat, fx, status = _solve(c)
            assert _kname() == "cc_solve_f16" + name, _kname()
            _against_truth(c, x_hat, fx, status, f"split {name} n={n} B={B}")


def test_overflowing_rows_on_the_unsplit_plan(dev):
    """tests/test_gpu_inverse.py::test_overflowing_rows_are_redone_on_bf16_pieces at a batch that runs one tile per wave, with
    overflowing rows in the first tile and in the five-lane tail tile: those rows hold the bf16x3 mode's numbers bit for bit, every
    other row -- their tile mates included -- the numbers of the fp16-piece launch without any overflowing row."""
    c = _case([50] * 4, 30, _unsplit_batch(4), 20, dev)
    B = c.B
    hot = torch.zeros(B, dtype=torch.bool, device=dev)
    hot[:12] = True
    hot[B - 3:] = True
    hot[B - 40] = True
    h = c.h.clone()
    h[hot] *= 3e6
    t = torch.randn(B, 1, generator=torch.Generator().manual_seed(2)).to(dev)
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
    assert not torch.equal(xs[~hot], xb[~hot]), "the two arithmetics differ in the last bits somewhere"
    assert not _flags(sf)[2].any() and not _flags(sf)[3].any()
    # the embedding really overflows fp16 pieces: the forward defers these rows too (equal to bf16x3), and only these
    umnn_amd.set_forward_precision("bf16x3")
    Fb = I.hip_forward(c.spec, None, xf, h, c.n)[0]
    umnn_amd.set_forward_precision("f16x3")
    Ff = I.hip_forward(c.spec, None, xf, h, c.n)[0]
    assert torch.equal(Ff[hot], Fb[hot]) and not torch.equal(Ff[16:B - 48], Fb[16:B - 48])


# ---- 3. stop rules and the status word ----------------------------------------------------------------------------------------
STOP = [([50] * 4, 30, p) for p in MODES] + [([100] * 3, 2, "f16x3")]
STOP_IDS = [f"{'x'.join(map(str, hid))}-{p}" for hid, _, p in STOP]


def _stop_case(hid, E, dev):
    """B = 100, n = 20; no |x| below 0.05, so that every |t| is far above 10 tol (min f is above 0.5 for these nets).  These nets are
    close to linear, so the first Newton point of many rows is already near the tolerance; seed 18 is one of the draws for which no
    row's float64 residual there lies within a factor five of tol = 1e-6, where fp32 rounding would decide whether the row goes on."""
    key = ("stop", tuple(hid), E)
    if key not in _CASES:
        base = _case(hid, E, 100, 20, dev, seed=18)
        c = copy.copy(base)
        c.xn = np.where(np.abs(base.xn) < 0.05, 0.05, base.xn)
        c.t64 = O.integrate_parallel(c.onet, np.zeros_like(c.xn), c.xn, c.hn, c.n)
        c.t = torch.from_numpy(c.t64).float().to(dev)
        c.f64 = O.integrand(c.onet, c.xn, c.hn)
        assert np.abs(c.t64).min() > 10 * 1e-6
        _CASES[key] = c
    return _CASES[key]


@pytest.mark.parametrize("hid,E,precision", STOP, ids=STOP_IDS)
def test_max_iter_1_returns_the_start_point_capped(hid, E, precision, dev):
    """One evaluation: x = clamp(0, lo, hi) exactly, evals = 1, CAPPED, f_x the integrand there.  On (0.5, 8) the rows whose solution
    lies below 0.5 are not capped: their one evaluation shows the target below G(lo) -- CLAMPED."""
    umnn_amd.set_forward_precision(precision)
    c = _stop_case(hid, E, dev)
    for lo, hi in ((-50., 50.), (0.5, 8.)):
        start = min(max(0., lo), hi)
        x_hat, fx, status = _solve(c, lo=lo, hi=hi, max_iter=1)
        evals, clamped, capped, nonfinite = _flags(status)
        assert torch.all(x_hat == start) and np.all(evals == 1) and not nonfinite.any()
        f0 = O.integrand(c.onet, np.full_like(c.xn, start), c.hn)
        assert U.rel_err(fx.cpu().numpy().reshape(-1, 1), f0) < TOL
        below = (c.xn < start - 0.01)[:, 0] if lo > 0 else np.zeros(c.B, bool)
        near = (np.abs(c.xn - start) <= 0.01)[:, 0] if lo > 0 else np.zeros(c.B, bool)
        assert np.all(clamped[below]) and not np.any(capped[below])
        assert np.all(capped[~below & ~near]) and not np.any(clamped[~below & ~near])
        if lo > 0:
            assert below.sum() > 10 and (~below & ~near).sum() > 10


@pytest.mark.parametrize("hid,E,precision", STOP, ids=STOP_IDS)
def test_max_iter_2_returns_the_first_newton_point(hid, E, precision, dev):
    """F(0) = 0, so the second point is x2 = t / f(0) (scale 1, offset 0), here from the float64 oracle.  |x - x2| <= 2 TOL max(1, |x2|):
    one TOL is the parity tolerance on f(0), the factor 2 covers the fp32 rounding of the step.  Rows whose float64 residual at x2
    already meets tol are left out; every other row has evals = 2, CAPPED and f_x = f(x).  With the draw of _stop_case no row is left
    out (and none is near enough to tol for fp32 rounding to decide it): the exclusion is kept for a draw that has such rows, and the
    premise is asserted first, so that a change of the default initialisation shows up as that and not as a kernel failure."""
    umnn_amd.set_forward_precision(precision)
    c = _stop_case(hid, E, dev)
    tol = 1e-6
    x2 = c.t64 / O.integrand(c.onet, np.zeros_like(c.xn), c.hn)
    res2 = np.abs(O.integrate_parallel(c.onet, np.zeros_like(x2), x2, c.hn, c.n) - c.t64)
    rel2 = (res2 / np.maximum(1., np.abs(c.t64)))[:, 0]
    keep = rel2 > tol
    assert np.all(np.abs(x2) < 50.) and not np.any((rel2 > tol / 5) & (rel2 < 5 * tol)), "the case's premise (see _stop_case)"
    x_hat, fx, status = _solve(c, tol=tol, max_iter=2)
    xh = x_hat.cpu().numpy().astype(np.float64)
    evals, clamped, capped, nonfinite = _flags(status)
    dev_x = np.abs(xh - x2) / (2 * TOL * np.maximum(1., np.abs(x2)))
    print(f"max_iter=2 {hid} {precision}: excluded {100. * (1 - keep.mean()):.1f} % of rows, max |x - x2| / bound {dev_x[keep].max():.3f}, "
          f"rows not capped among the kept {int((~capped[keep]).sum())}")
    assert keep.mean() > 0.95
    assert np.all(dev_x[keep] <= 1.), np.flatnonzero(dev_x[:, 0] > 1.)
    assert np.all(evals[keep] == 2) and np.all(capped[keep]) and not clamped.any() and not nonfinite.any()
    assert U.rel_err(fx.cpu().numpy().reshape(-1, 1)[keep], O.integrand(c.onet, xh, c.hn)[keep]) < TOL


@pytest.mark.parametrize("hid,E,precision", STOP, ids=STOP_IDS)
def test_tol_0_ends_by_bracket_collapse_not_by_the_cap(hid, E, precision, dev):
    """tol = 0 leaves the two other stop rules: the bracket has collapsed to adjacent floats, or x has stopped changing.  No row is
    capped at max_iter = 64 and the error stays within the bound (the fp32 reference iteration needs at most 10 evaluations)."""
    umnn_amd.set_forward_precision(precision)
    c = _stop_case(hid, E, dev)
    x_hat, fx, status = _solve(c, tol=0., max_iter=64)
    print(f"tol=0 {hid} {precision}: evaluations <= {_flags(status)[0].max()}")
    _against_truth(c, x_hat, fx, status, f"tol=0 {hid} {precision}")


@pytest.mark.parametrize("hid,E,precision", STOP, ids=STOP_IDS)
def test_evaluation_counts_match_the_float64_iteration(hid, E, precision, dev):
    """The status word's count against tests/_inverse_truth.newton64 (the iteration of include/umnn_cc.h in float64) at the default
    settings: within one evaluation, row by row."""
    umnn_amd.set_forward_precision(precision)
    c = _stop_case(hid, E, dev)
    key = ("newton64", tuple(hid), E)
    if key not in _CASES:
        _CASES[key] = T.newton64(T.integral_map(c.onet, c.hn, c.n), c.t64)
    x64, e64, clamped64, capped64 = _CASES[key]
    assert not clamped64.any() and not capped64.any() and np.max(np.abs(x64 - c.xn)) <= 1e-6 / c.f64.min() * 2
    x_hat, fx, status = _solve(c)
    evals = _flags(status)[0].astype(np.int64)
    diff = evals - e64[:, 0]
    print(f"evaluations {hid} {precision}: kernel {evals.min()}..{evals.max()}, float64 {e64.min()}..{e64.max()}, "
          f"kernel - float64 in [{diff.min()}, {diff.max()}]")
    assert np.abs(diff).max() <= 1
    _against_truth(c, x_hat, fx, status, f"default settings {hid} {precision}")


@pytest.mark.parametrize("hid,E,precision", STOP, ids=STOP_IDS)
def test_want_info_false_returns_the_same_x(hid, E, precision, dev):
    """Null f_x / status pointers change nothing about x."""
    umnn_amd.set_forward_precision(precision)
    c = _stop_case(hid, E, dev)
    x_info, fx, status = _solve(c)
    x_bare, none_fx, none_status = _solve(c, want_info=False)
    assert none_fx is None and none_status is None and fx is not None and status is not None
    assert torch.equal(x_bare, x_info)


# ---- 4. non-finite inputs ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", MODES)
def test_nan_rows_come_back_nan_and_nothing_else_does(precision, dev):
    """A NaN target (rows 3 and 40) or a NaN in the embedding (row 20) returns NaN with NONFINITE -- under fp16 pieces through the
    deferral to the queued bf16 build, which then has nothing finite to put there.  Every other row, the lanes sharing a tile with
    those rows included, holds the bits of the same launch with finite values in those rows."""
    umnn_amd.set_forward_precision(precision)
    c = _case([50] * 4, 30, 50, 20, dev)
    bad = [3, 20, 40]
    t, h = c.t.clone(), c.h.clone()
    t[3], t[40] = float("nan"), float("nan")
    h[20, 7] = float("nan")
    x_ref, fx_ref, s_ref = _solve(c)
    x_out = torch.full((c.B, 1), 5.0, device=dev)
    out = I.hip_solve(c.spec, h, t, c.n, x_out=x_out)
    assert out is not None and out[0] is x_out and _kname().startswith("cc_solve_")
    _, fx, status = out
    evals, clamped, capped, nonfinite = _flags(status)
    good = np.setdiff1d(np.arange(c.B), bad)
    assert torch.isnan(x_out[bad]).all() and nonfinite[bad].all() and not capped[bad].any() and not clamped[bad].any()
    assert not nonfinite[good].any()
    assert torch.equal(x_out[good], x_ref[good]) and torch.equal(fx[good], fx_ref[good]) and torch.equal(status[good], s_ref[good])
    _against_truth(c, x_out, fx, status, f"rows next to NaN rows {precision}", rows=good)


@pytest.mark.parametrize("precision", MODES)
def test_infinite_targets_end_on_the_endpoints_and_only_column_j_is_written(precision, dev):
    """+inf lies above G(hi), -inf below G(lo): hi / lo with CLAMPED, on the default bracket and on (-4, 6).  The output is column 1 of a
    [B, 3] buffer of NaN: columns 0 and 2 stay NaN."""
    umnn_amd.set_forward_precision(precision)
    c = _case([50] * 4, 30, 50, 20, dev)
    d, j = 3, 1
    t = torch.zeros(c.B, d, device=dev)
    t[:, j] = c.t[:, 0]
    up, down = [0, 17, 49], [5, 16, 33]
    t[up, j], t[down, j] = float("inf"), float("-inf")
    h = torch.zeros(c.B, c.E, d, device=dev)
    h[:, :, j] = c.h
    h = h.view(c.B, c.E * d).contiguous()
    x_ref = _solve(c)[0]
    for lo, hi in ((-50., 50.), (-4., 6.)):
        x_out = torch.full((c.B, d), float("nan"), device=dev)
        out = I.hip_solve(c.spec, h, t, c.n, j=j, lo=lo, hi=hi, x_out=x_out)
        assert out is not None and out[0] is x_out
        evals, clamped, capped, nonfinite = _flags(out[2])
        assert torch.isnan(x_out[:, [0, 2]]).all(), "only column j is written"
        assert torch.all(x_out[up, j] == hi) and torch.all(x_out[down, j] == lo)
        assert clamped[up].all() and clamped[down].all() and not capped.any() and not nonfinite.any()
        rest = np.setdiff1d(np.arange(c.B), up + down)
        inside = rest[(c.xn[rest, 0] > lo + 0.01) & (c.xn[rest, 0] < hi - 0.01)]
        assert not clamped[inside].any() and len(inside) > 40
        if lo == -50.:
            assert torch.equal(x_out[rest, j], x_ref[rest, 0]), "the stride-d operands give the bits of the plain [B, 1] call"
        bound = TOL / float(c.f64[inside].min())
        assert float(np.max(np.abs(x_out[inside, j].cpu().numpy() - c.xn[inside, 0]))) <= bound


# ---- 5. brackets ---------------------------------------------------------------------------------------------------------------
BRACKETS = [(-4., 6.), (0.5, 8.), (-8., -0.5), (0.25, 0.75)]


def _bracket_case(dev):
    """B = 100 with four rows moved beyond the ends of every bracket above, so that each has rows on both sides."""
    key = ("bracket",)
    if key not in _CASES:
        base = _case([50] * 4, 30, 100, 20, dev, seed=5)
        c = copy.copy(base)
        c.xn = base.xn.copy()
        c.xn[:4, 0] = [-9., 9., -4.5, 6.5]
        c.t64 = O.integrate_parallel(c.onet, np.zeros_like(c.xn), c.xn, c.hn, c.n)
        c.t = torch.from_numpy(c.t64).float().to(dev)
        c.f64 = O.integrand(c.onet, c.xn, c.hn)
        _CASES[key] = c
    return _CASES[key]


def _check_bracket(xh, clamped, capped, nonfinite, x_true, sf, lo, hi, tag):
    """Rows whose solution lies inside (lo, hi): the truth bound, no CLAMPED.  Rows outside: the endpoint exactly, CLAMPED.  A row
    within the bound of an endpoint may be either (its target is within the parity tolerance of G(endpoint)): it is held to the
    bound against the nearer of the two."""
    bound = TOL / float(sf.min())
    inside = (x_true > lo + bound) & (x_true < hi - bound)
    left, right = x_true < lo - bound, x_true > hi + bound
    err = np.abs(xh - np.clip(x_true, lo, hi))
    print(f"{tag} [{lo}, {hi}]: {inside.sum()} rows inside ({100. * inside.mean():.1f} %), {left.sum()} below, {right.sum()} above, "
          f"|x_hat - x| {err.max():.2e} (bound {bound:.2e})")
    assert inside.any() and left.any() and right.any()
    assert err.max() <= bound
    assert np.all(xh[left] == np.float32(lo)) and np.all(xh[right] == np.float32(hi)) and clamped[left | right].all()
    assert not clamped[inside].any() and not capped.any() and not nonfinite.any()
    return inside


@pytest.mark.parametrize("precision", MODES)
@pytest.mark.parametrize("lo,hi", BRACKETS)
def test_brackets_that_exclude_zero_and_narrow_ones(lo, hi, precision, dev):
    """The start point is 0 clamped into the bracket; an endpoint is tried once when a step overshoots it."""
    umnn_amd.set_forward_precision(precision)
    c = _bracket_case(dev)
    x_hat, fx, status = _solve(c, lo=lo, hi=hi)
    xh = x_hat.cpu().numpy().astype(np.float64)[:, 0]
    evals, clamped, capped, nonfinite = _flags(status)
    inside = _check_bracket(xh, clamped, capped, nonfinite, c.xn[:, 0], c.f64[:, 0], lo, hi, f"{precision}")
    assert evals.max() <= 12 and evals.min() >= 1
    res = np.abs(O.integrate_parallel(c.onet, np.zeros_like(c.xn), xh[:, None], c.hn, c.n) - c.t64) / np.maximum(1., np.abs(c.t64))
    assert res[inside].max() <= TOL
    assert U.rel_err(fx.cpu().numpy()[:, None], O.integrand(c.onet, xh[:, None], c.hn)) < TOL, "f_x is the integrand at the returned x"


def _g5(n, dev):
    G = U.load(f"g5_monotonic_n{n}")
    m = umnn_amd.MonotonicNN(3, [100, 100, 100], nb_steps=n, dev=dev)
    m.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in U.state_dict_of(G).items()})
    m.to(dev)
    net, cW, cb = T.monotonic_parts(G)
    sf = T.monotonic_map(net, cW, cb, G["h"], n)(G["x"].astype(np.float64))[1]
    return G, m, sf


def _bracket_of(x):
    """A bracket around the middle half of the fixture's solutions: a quarter of the rows beyond either end."""
    return float(np.round(np.quantile(x, 0.25), 2)), float(np.round(np.quantile(x, 0.75), 2))


@pytest.mark.parametrize("precision", ["f16x3", "fp32"])
def test_monotonic_inverse_with_an_x_range(precision, dev):
    umnn_amd.set_forward_precision(precision)
    G, m, sf = _g5(50, dev)
    lo, hi = _bracket_of(G["x"])
    with torch.no_grad():
        x_hat, fx, status = m.inverse(torch.from_numpy(G["y"]).to(dev), torch.from_numpy(G["h"]).to(dev), x_range=(lo, hi),
                                      return_info=True)
    assert umnn_amd.path_taken() == "hip" and _kname().startswith("cc_solve_f16<T=7,EXACT=1,LIVE=26,WAVES=8>"), _kname()
    evals, clamped, capped, nonfinite = _flags(status)
    _check_bracket(x_hat.cpu().numpy().astype(np.float64)[:, 0], clamped[:, 0], capped, nonfinite, G["x"].astype(np.float64)[:, 0], sf[:, 0],
                   lo, hi, f"MonotonicNN.inverse {precision}")


@pytest.mark.parametrize("precision", ["f16x3", "bf16x3"])
def test_per_row_scale_and_offset_operands(precision, dev):
    """The scale_row / off_row form of the entry point: the kernel solves exp(s(h)) (o'(h) + int_0^x f) = y with the conditioner's
    per-row scale and offset as operands, on the whole range and on a bracket with rows beyond both ends."""
    umnn_amd.set_forward_precision(precision)
    G, m, sf = _g5(50, dev)
    y, h = torch.from_numpy(G["y"]).to(dev), torch.from_numpy(G["h"]).to(dev)
    with torch.no_grad():
        out = m.net(h)
        scale = torch.exp(out[:, 1]).contiguous()
        off = (out[:, 0] / scale).contiguous()                   # y = scale (off + F)  <=>  y = scale F + o
    spec = mlp_spec(m.integrand)
    x_true = G["x"].astype(np.float64)[:, 0]
    for lo, hi in ((-50., 50.), _bracket_of(G["x"])):
        res = I.hip_solve(spec, h, y, 50, scale_row=scale, off_row=off, lo=lo, hi=hi)
        assert res is not None and _kname().endswith("<T=7,EXACT=1,LIVE=26,WAVES=8>"), _kname()
        x_hat, fx, status = res
        evals, clamped, capped, nonfinite = _flags(status)
        xh = x_hat.cpu().numpy().astype(np.float64)[:, 0]
        if lo == -50.:
            bound = TOL / float(sf.min())
            print(f"scale_row / off_row {precision}: |x_hat - x| {np.abs(xh - x_true).max():.2e} (bound {bound:.2e})")
            assert np.abs(xh - x_true).max() <= bound and not clamped.any() and not capped.any() and not nonfinite.any()
        else:
            _check_bracket(xh, clamped, capped, nonfinite, x_true, sf[:, 0], lo, hi, f"scale_row / off_row {precision}")
        net = T.monotonic_parts(G)[0]
        assert U.rel_err(fx.cpu().numpy()[:, None], O.integrand(net, xh[:, None], G["h"].astype(np.float64))) < TOL


# ---- 6. the flow path ----------------------------------------------------------------------------------------------------------
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


@pytest.mark.parametrize("precision", MODES)
def test_newton_round_trip_of_a_conditional_flow(precision, dev):
    """invert(method="newton", context=c) on a flow shaped like the g4_flow2_cond fixture (ConditionnalMADE): the conditioner runs in
    full for every dimension, then one solve launch."""
    umnn_amd.set_forward_precision(precision)
    torch.manual_seed(23)
    d, nb_flow, cond, B = 3, 2, 3, 33
    m = umnn_amd.UMNNMAFFlow(nb_flow=nb_flow, nb_in=d, hidden_derivative=[50] * 4, hidden_embedding=[48, 48], embedding_s=30,
                             nb_steps=20, solver="CCParallel", cond_in=cond).to(dev).eval()
    with torch.no_grad():
        for blk in m.nets:
            for mod in blk.net.parallel_nets.net:
                if isinstance(mod, torch.nn.Linear):
                    mod.weight.mul_(1.5)
    x = torch.randn(B, d, device=dev) * 1.5
    ctx = torch.randn(B, cond, device=dev)
    bound = _flow_bound(m, x, ctx)
    with torch.no_grad():
        z = m(x, context=ctx)
        before = _lib.lib().umnn_launch_count()
        x_newton = m.invert(z, method="newton", context=ctx)
        assert _lib.lib().umnn_launch_count() - before == nb_flow * d, "exactly one solve launch per dimension and block"
        assert umnn_amd.path_taken() == "hip" and _kname().startswith("cc_solve_") and "T=4" in _kname() and "LIVE=13" in _kname(), _kname()
        z2 = m(x_newton, context=ctx)
        x_other = m.invert(z, method="newton", context=torch.flip(ctx, [0]))
    err = float((x_newton - x).abs().max())
    print(f"conditional flow {precision}: newton {err:.2e}, bound {bound:.2e}")
    assert err <= bound
    assert U.rel_err(z2.cpu().numpy(), z.cpu().numpy()) < TOL
    assert float((x_other - x).abs().max()) > 100 * bound, "the context is really read"


def test_newton_with_bf16_embedding_matches_fp32_embedding(dev):
    """tests/test_gpu_round3.py::test_invert_with_bf16_embedding_matches_fp32_embedding for method="newton": the embedding is widened to
    fp32 for the solve; samples agree with the fp32-embedding ones to the embedding's rounding and round-trip through forward."""
    torch.manual_seed(5)
    d = 6
    model = umnn_amd.UMNNMAFFlow(nb_flow=2, nb_in=d, hidden_derivative=[50] * 3, hidden_embedding=[64, 64], embedding_s=8,
                                 nb_steps=30, solver="CCParallel").to(dev).eval()
    z = torch.randn(200, d, device=dev)
    with torch.no_grad():
        before = _lib.lib().umnn_launch_count()
        x32 = model.invert(z, method="newton")
        assert umnn_amd.path_taken() == "hip" and _lib.lib().umnn_launch_count() - before == 2 * d
        model.set_embedding_dtype(torch.bfloat16)
        try:
            before = _lib.lib().umnn_launch_count()
            x16 = model.invert(z, method="newton")
            assert _lib.lib().umnn_launch_count() - before == 2 * d and _kname().startswith("cc_solve_"), _kname()
            assert model.nets[0].net.m_embeding.dtype == torch.bfloat16
            z_back = model.forward(x16)
        finally:
            model.set_embedding_dtype(None)
    assert torch.isfinite(x16).all() and not torch.equal(x16, x32)
    assert float((x16 - x32).abs().max()) < 5e-2 * max(1.0, float(x32.abs().max()))
    assert float((z_back - z).abs().max()) < 5e-2 * max(1.0, float(z.abs().max()))
