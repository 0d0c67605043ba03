"""The in-kernel bracket search (umnn_flow_invert_dim, the default of UMNNMAFFlow.invert) called directly through
integral.hip_invert_dim: every reachable row of kInvVariants / kInvWideFirst (cc_invert.hip) by name in both builds, both launch plans
(one sample per wave / one sample per workgroup with the node range split over its waves), the round counts 1 and 10, which columns
are read and written, targets outside the range, the fp16-piece overflow protocol, non-finite inputs and determinism.

Truth (tests/_bracket_truth.py): targets z64 = exp(scaling_j) (h[:, 0 d + j] + int_0^x f) from the float64 oracle, and a float64
restatement of the search on the kernel's fp32 candidate grid.  TOL = 1e-4 is the forward parity tolerance of the project.
  (a) |x_hat - x| <= 100 / 9^iters + TOL max(1, |z|) / (exp(scaling_j) min f): the bracket after k rounds is one candidate step of
      round k wide (100 / 9^k) and holds the solution unless a decision was taken on an image that is off by more than TOL;
  (b) x_hat is the restatement's candidate to one fp32 ulp of 50 on every row whose decision margin exceeds TOL max(1, |z|); the
      rows left out are at most 10 % of the batch (tests/test_bracket_cpu.py confirms both with the host-driven fp32 search).
Inputs (tests/_bracket_truth.case): default-initialised IntegrandNetwork(3, 1 + E, hid, 1), x ~ 1.5 N(0, 1), h ~ N(0, 1), scaling ~
0.3 N(0, 1), d = 3 with j over {0, 2}; x_inv is prefilled with a sentinel."""
import copy
import types

import numpy as np
import pytest
import torch

import umnn_amd
from tests import _bracket_truth as BT
from tests._bracket_truth import BIG, FAMILIES, FAMILY_IDS, FLOW_NAME, JS, SPLIT_EDGES, STEP6, TOL, VARIANTS
from tests.test_gpu_solve_coverage import _unsplit_batch
from umnn_amd import _lib, integral as I
from umnn_amd.nets import mlp_spec

pytestmark = pytest.mark.gpu
MODES = ["f16x3", "bf16x3", "bf16x6", "fp32"]
D = BT.D
SENTINEL = -777.25


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


def _cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


_ON_DEVICE = {}


def _case(hid, E, B, n, dev, seed=None):
    """The shared CPU case (inputs and float64 truth, cached and never modified) with a copy of its net and inputs on the device."""
    c = BT.case(hid, E, B, n, BT.seed_of(hid, E) if seed is None else seed)
    if id(c) not in _ON_DEVICE:
        net = copy.deepcopy(c.net).to(dev)
        _ON_DEVICE[id(c)] = types.SimpleNamespace(c=c, net=net, spec=mlp_spec(net), h=c.h.to(dev), z=c.z.to(dev),
                                                  scaling=c.scaling.to(dev))
    return c, _ON_DEVICE[id(c)]


def _invert(g, j, iters, name, z=None, h=None):
    """One launch of the kernel ``name`` (asserted) through the C entry point into a [B, D] buffer of sentinels -> that buffer."""
    z = g.z if z is None else z
    x_inv = torch.full((z.shape[0], D), SENTINEL, device=z.device)
    before = _lib.lib().umnn_launch_count()
    ok = I.hip_invert_dim(g.spec, g.h if h is None else h, z, g.scaling, g.c.n, j, iters, x_inv)
    assert ok is True and umnn_amd.path_taken() == "hip" and _lib.lib().umnn_launch_count() - before == 1
    assert _kname() == name, (_kname(), name)
    return x_inv


def _bits(t):
    return t.contiguous().view(torch.int32)


def _same_bits(a, b):
    return torch.equal(_bits(a), _bits(b))


def _check_a(c, x_col, j, step, tag, rows=slice(None)):
    """Check (a) on ``rows`` of column j -> max |x_hat - x| / bound."""
    xh = x_col.cpu().numpy().astype(np.float64)
    assert np.isfinite(xh).all(), tag
    ratio = float(np.max(np.abs(xh - c.xn[rows, j]) / BT.truth_bound(c, j, step, TOL, rows)))
    print(f"(a) {tag} j={j}: max |x_hat - x| / bound = {ratio:.3f}")
    assert ratio <= 1., tag
    return ratio


def _check_b(c, x_col, j, iters, tag):
    """Check (b) on column j -> share of the rows left out."""
    best, margin = BT.truth(c, j, iters)
    keep = margin > TOL * np.maximum(1., np.abs(c.z[:, j].double().numpy()))
    off = np.abs(x_col.cpu().numpy().astype(np.float64) - best.astype(np.float64)) > BT.ULP_50
    share = 1. - float(keep.mean())
    print(f"(b) {tag} j={j} iters={iters}: left out {100. * share:.1f} % of {c.B} rows ({int(off[~keep].sum())} of them differ), "
          f"kept rows that differ: {int(off[keep].sum())}")
    assert share <= 0.10, tag
    assert not off[keep].any(), (tag, np.flatnonzero(off & keep))
    return share


# ---- 1. every row of both variant tables, by name, on both launch plans (tables: tests/_bracket_truth.py) -------------------------
@pytest.mark.parametrize("precision,name,hid,E", VARIANTS, ids=[f"{p}-{'x'.join(map(str, hid))}" for p, _, hid, _ in VARIANTS])
def test_every_table_row_by_name_on_both_plans(precision, name, hid, E, dev):
    """B = 37 samples on the kernel the plan names for this net: few enough for the split plan on any device.  n = 20: the node range
    is split over the workgroup's waves.  n = 2: fewer nodes than waves, so the same rows run one sample per wave."""
    umnn_amd.set_forward_precision(precision)
    for n in (20, 2):
        c, g = _case(hid, E, 37, n, dev)
        for j in JS:
            tag = f"{name} {precision} n={n}"
            _check_a(c, _invert(g, j, 6, name)[:, j], j, STEP6, tag)
            _check_b(c, _invert(g, j, 4, name)[:, j], j, 4, tag)


# ---- 2. one round and the default ten ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision,name,hid,E", FAMILIES, ids=FAMILY_IDS)
def test_one_round_returns_a_first_round_candidate(precision, name, hid, E, dev):
    """iters = 1: one of the ten candidates fl(fl(p / 9) 100) - 50 on every row -- to one fp32 ulp of 50, the measure of check (b): the
    compiled kernel forms them with one fma -- and the restatement's on the rows that are not marginal."""
    umnn_amd.set_forward_precision(precision)
    first = (np.arange(10) / 9.0).astype(np.float32) * np.float32(100.) + np.float32(-50.)
    c, g = _case(hid, E, 37, 20, dev)
    for j in JS:
        x = _invert(g, j, 1, name)[:, j]
        assert np.all(np.abs(x.cpu().numpy().astype(np.float64)[:, None] - first.astype(np.float64)[None, :]).min(axis=1) <= BT.ULP_50)
        _check_b(c, x, j, 1, f"{name} {precision}")


@pytest.mark.parametrize("precision,name,hid,E", FAMILIES, ids=FAMILY_IDS)
def test_ten_rounds_end_within_the_forward_tolerance(precision, name, hid, E, dev):
    """iters = 10, the API default: 100 / 9^10 is below the fp32 spacing of the bracket's ends, the search has collapsed (ties go to the
    lower candidate), and what is left of (a) is its second term."""
    umnn_amd.set_forward_precision(precision)
    c, g = _case(hid, E, 37, 20, dev)
    for j in JS:
        _check_a(c, _invert(g, j, 10, name)[:, j], j, 0., f"iters=10 {name} {precision}")


# ---- 3. both launch plans --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hid,E,wpb,name", SPLIT_EDGES, ids=[n for _, _, _, n in SPLIT_EDGES])
def test_split_plan_at_the_edges_of_the_node_partition(hid, E, wpb, name, dev):
    """Wave `part` of wpb sums nodes [part (n + 1) / wpb, (part + 1) (n + 1) / wpb): n + 1 = wpb gives every wave one node, wpb + 1 an
    uneven split, wpb + 2 another; one sample, sixteen, seventeen."""
    for n in (wpb - 1, wpb, wpb + 1):
        for B in (1, 16, 17):
            c, g = _case(hid, E, B, n, dev, seed=0)
            for j in JS:
                _check_a(c, _invert(g, j, 6, name)[:, j], j, STEP6, f"split {name} n={n} B={B}")


BIG_RUNS = [("flow_50x4", p) for p in MODES] + [("waves8_100x3", "f16x3"), ("wide_first", "f16x3")]


@pytest.mark.parametrize("net_name,precision", BIG_RUNS)
def test_unsplit_plan_on_every_row_of_a_large_batch(net_name, precision, dev):
    """More samples than the split plan accepts (B wpb > 8 CUs): one sample per wave.  Every row against the truth, the last five rows
    on their own as well; the first 48 rows launched alone take the split plan and agree with the large launch within the bound."""
    umnn_amd.set_forward_precision(precision)
    hid, E, wpb, names = BIG[net_name]
    name = names[precision]
    c, g = _case(hid, E, _unsplit_batch(wpb), 20, dev, seed=0)
    assert c.B * wpb > 8 * _cus()
    for j in JS:
        x_big = _invert(g, j, 6, name)[:, j]
        tag = f"unsplit {net_name} B={c.B} {precision}"
        _check_a(c, x_big, j, STEP6, tag)
        _check_a(c, x_big[c.B - 5:], j, STEP6, tag + " last five rows", rows=slice(c.B - 5, c.B))
        x_small = _invert(g, j, 6, name, z=g.z[:48].contiguous(), h=g.h[:48].contiguous())[:, j]
        _check_a(c, x_small, j, STEP6, tag + " first 48 rows alone", rows=slice(0, 48))
        assert np.all(np.abs((x_small - x_big[:48]).cpu().numpy().astype(np.float64)) <= BT.truth_bound(c, j, STEP6, TOL, slice(0, 48)))
        print(f"{tag} j={j}: split and unsplit plan differ in some bit: {not _same_bits(x_small, x_big[:48])}")


def test_the_boundary_between_the_two_plans(dev):
    """B wpb = 8 CUs is the last batch of the split plan, one sample more the first of the unsplit one: both within (a), and the shared
    rows agree within the bound."""
    hid, E, wpb, names = BIG["flow_50x4"]
    name = names["f16x3"]
    B0 = 8 * _cus() // wpb
    c, g = _case(hid, E, B0 + 1, 20, dev, seed=0)
    for j in JS:
        x_over = _invert(g, j, 6, name)[:, j]
        x_at = _invert(g, j, 6, name, z=g.z[:B0].contiguous(), h=g.h[:B0].contiguous())[:, j]
        _check_a(c, x_over, j, STEP6, f"B = 8 CUs / wpb + 1 = {B0 + 1}")
        _check_a(c, x_at, j, STEP6, f"B = 8 CUs / wpb = {B0}", rows=slice(0, B0))
        assert np.all(np.abs((x_at - x_over[:B0]).cpu().numpy().astype(np.float64)) <= BT.truth_bound(c, j, STEP6, TOL, slice(0, B0)))
        print(f"plan boundary j={j}: the two launches differ in some bit: {not _same_bits(x_at, x_over[:B0])}")


def _both_plans():
    """(batch of the split plan, batch of the unsplit plan) for the four-wave kernels on this device."""
    return 37, 8 * _cus() // 4 + 5


# ---- 4. which columns are read and written -------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", MODES)
def test_only_column_j_is_read_and_written(precision, dev):
    """After a launch for column j every other column of x_inv holds the sentinel bit for bit; other h[:, e d + j'] and z[:, j'], j' != j,
    leave column j bit-identical."""
    umnn_amd.set_forward_precision(precision)
    for B in _both_plans():
        c, g = _case([50] * 4, 30, B, 20, dev, seed=0)
        gen = torch.Generator().manual_seed(B)
        for j in range(D):
            x_ref = _invert(g, j, 6, FLOW_NAME[precision])
            others = [k for k in range(D) if k != j]
            assert torch.all(_bits(x_ref[:, others]) == _bits(torch.tensor([SENTINEL]))[0].item())
            assert torch.isfinite(x_ref[:, j]).all() and not torch.any(x_ref[:, j] == SENTINEL)
            h3 = g.h.clone().view(B, c.E, D)
            z = g.z.clone()
            for k in others:
                h3[:, :, k] = torch.randn(B, c.E, generator=gen).to(dev) * 3.
                z[:, k] = torch.randn(B, generator=gen).to(dev) * 3.
            x_new = _invert(g, j, 6, FLOW_NAME[precision], z=z, h=h3.view(B, c.E * D))
            assert _same_bits(x_new, x_ref)


# ---- 5. targets outside the range, overflow, non-finite inputs, determinism ---------------------------------------------------
@pytest.mark.parametrize("precision", MODES)
def test_targets_outside_the_range_end_on_its_ends(precision, dev):
    """z = +-1e6 lies beyond G(+-50): exactly +-50.  Every other row holds the bits of the launch without those targets."""
    umnn_amd.set_forward_precision(precision)
    for B in _both_plans():
        c, g = _case([50] * 4, 30, B, 20, dev, seed=0)
        up, down = [0, 17, B - 1], [5, 16, B - 4]
        rest = np.setdiff1d(np.arange(B), up + down)
        for j in JS:
            x_ref = _invert(g, j, 6, FLOW_NAME[precision])
            z = g.z.clone()
            z[up, j], z[down, j] = 1e6, -1e6
            x = _invert(g, j, 6, FLOW_NAME[precision], z=z)
            assert torch.all(x[up, j] == 50.) and torch.all(x[down, j] == -50.)
            assert _same_bits(x[rest], x_ref[rest])


def test_overflowing_samples_are_redone_on_bf16_pieces(dev):
    """The recipe of tests/test_gpu_solve_coverage.py::test_overflowing_rows_on_the_unsplit_plan on both plans: an embedding scaled by
    3e6 overflows the fp16 pieces.  Those samples are finite and hold the bf16x3 mode's numbers bit for bit, every other sample the
    numbers of the fp16-piece launch without any overflowing sample.  Ten rounds, so that the two arithmetics can differ at all."""
    for B in _both_plans():
        c, g = _case([50] * 4, 30, B, 20, dev, seed=0)
        hot = torch.zeros(B, dtype=torch.bool, device=dev)
        hot[:3] = True
        hot[B - 3:] = True
        hot[B // 2] = True
        for j in JS:
            h3 = g.h.clone().view(B, c.E, D)
            h3[hot, :, j] *= 3e6
            h = h3.view(B, c.E * D)
            umnn_amd.set_forward_precision("bf16x3")
            xb = _invert(g, j, 10, FLOW_NAME["bf16x3"], h=h)[:, j]
            umnn_amd.set_forward_precision("f16x3")
            xf = _invert(g, j, 10, FLOW_NAME["f16x3"], h=h)[:, j]
            xs = _invert(g, j, 10, FLOW_NAME["f16x3"])[:, j]            # (no overflowing sample)
            assert torch.isfinite(xf).all()
            assert _same_bits(xf[hot], xb[hot]) and _same_bits(xf[~hot], xs[~hot])
            assert not _same_bits(xs[~hot], xb[~hot]), "the two arithmetics differ in the last bits somewhere"


@pytest.mark.parametrize("precision", MODES)
def test_nan_rows_come_back_nan_and_nothing_else_does(precision, dev):
    """A NaN in the embedding of dimension j (the offset row, another row) or a NaN target returns NaN -- under fp16 pieces through
    the deferral to the queued bf16 build, which has nothing finite to put there either.  Every other sample holds the bits of the
    launch without them."""
    umnn_amd.set_forward_precision(precision)
    for B in _both_plans():
        c, g = _case([50] * 4, 30, B, 20, dev, seed=0)
        bad = [3, 20, B - 2, B - 1]
        good = np.setdiff1d(np.arange(B), bad)
        for j in JS:
            x_ref = _invert(g, j, 6, FLOW_NAME[precision])
            h3 = g.h.clone().view(B, c.E, D)
            z = g.z.clone()
            h3[3, 7, j] = float("nan")
            h3[B - 2, 0, j] = float("nan")
            z[20, j], z[B - 1, j] = float("nan"), float("nan")
            x = _invert(g, j, 6, FLOW_NAME[precision], z=z, h=h3.view(B, c.E * D))
            assert torch.isnan(x[bad, j]).all(), x[bad, j]
            assert _same_bits(x[good], x_ref[good]) and torch.isfinite(x[good, j]).all()


@pytest.mark.parametrize("precision", ["f16x3", "fp32"])
def test_two_identical_launches_return_the_same_bits(precision, dev):
    umnn_amd.set_forward_precision(precision)
    for B in _both_plans():
        c, g = _case([50] * 4, 30, B, 20, dev, seed=0)
        for j in JS:
            assert _same_bits(_invert(g, j, 10, FLOW_NAME[precision]), _invert(g, j, 10, FLOW_NAME[precision]))
