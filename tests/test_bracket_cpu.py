"""The bracket search without a GPU: the float64 restatement (tests/_bracket_truth.py) against the recorded fixture and against its
own provable resolution, and the package's host-driven fp32 search (UMNNMAF._invert on ATen under integral.force_generic()) on the
inputs of tests/test_gpu_invert_coverage.py -- the confirmation that the reference arithmetic alone stays inside the bound (a) and
the share cap of check (b) that the kernels are held to there."""
import numpy as np
import pytest
import torch

import umnn_amd
from tests import _bracket_truth as BT
from tests import _inverse_truth as T
from tests import _util as U
from umnn_amd import integral

TOL = BT.TOL
NETS = sorted({(tuple(hid), E) for _, _, hid, E in BT.VARIANTS})


def test_restatement_reproduces_the_recorded_fixture():
    """g6_invert: x_inv recorded from the reference's invert(z, iter=5) on a two-block flow.  The restatement chained through the
    oracle's MADE for both blocks reproduces it within the two last-round candidate steps test_invert_on_gpu_matches_reference uses."""
    G = U.load("g6_invert")
    blocks = T.blocks_from_state_dict(U.state_dict_of(G), 2)
    x = BT.flow_bracket64(blocks, G["z"], 30, 5)
    err = float(np.max(np.abs(x - G["x_inv"])))
    print(f"g6_invert: |restatement - recorded x_inv| {err:.2e}, |restatement - x| {float(np.max(np.abs(x - G['x']))):.2e}")
    assert err < 2 * 100. / 9 ** 5
    assert float(np.max(np.abs(x - G["x"]))) < 2 * 100. / 9 ** 5


@pytest.mark.parametrize("iters", [4, 5, 6, 8])
def test_resolution_of_the_search_is_one_candidate_step(iters):
    """In float64 the returned candidate is an end of a bracket 100 / 9^iters wide that holds the solution: |x_hat - x| <= 100 / 9^iters
    (not the 100 (2/9)^iters of a bracket two steps wide)."""
    c = BT.case([50] * 4, 30, 64, 20)
    for j in range(BT.D):
        x, _ = BT.bracket64(c.onet, c.hn.reshape(c.B, c.E, BT.D)[:, :, j], c.z64[:, j], c.sn[j], c.n, iters)
        err = float(np.max(np.abs(x - c.xn[:, j])))
        print(f"iters={iters} j={j}: max |x_hat - x| = {err:.2e} = {err * 9 ** iters / 100.:.2f} steps")
        assert err <= 100. / 9 ** iters * (1 + 1e-9)


def test_every_table_row_is_named_or_listed_as_unreachable():
    """kInvVariants: 15 two-piece rows in two builds and 4 three-piece rows; kInvWideFirst: 8 rows in two builds."""
    named = {name for _, name, _, _ in BT.VARIANTS}
    listed = {name for name, _ in BT.UNREACHABLE}
    assert not named & listed and len(named | listed) == 15 * 2 + 4 + 8 * 2


class _FixedEmbedding(torch.nn.Module):
    """The conditioner of a UMNNMAF block with its output pinned to the case's h."""

    def __init__(self, integrand, h):
        super().__init__()
        self.parallel_nets = integrand
        self.h = h

    def make_embeding(self, x, context=None):
        return self.h


def _host_search(c, iters):
    m = umnn_amd.UMNNMAF(_FixedEmbedding(c.net, c.h), BT.D, nb_steps=c.n, solver="CCParallel")
    with torch.no_grad():
        m.scaling.copy_(c.scaling)
        with integral.force_generic():
            x = m.invert(c.z, iter=iters)
    assert umnn_amd.path_taken() == "aten"
    return x.numpy().astype(np.float64)


def _check_b(c, x, j, iters):
    best, margin = BT.truth(c, j, iters)
    keep = margin > TOL * np.maximum(1., np.abs(c.z[:, j].double().numpy()))
    off = np.abs(x[:, j] - best.astype(np.float64)) > BT.ULP_50
    return 1. - float(keep.mean()), int(off[keep].sum()), int(off[~keep].sum())


@pytest.mark.parametrize("hid,E", NETS, ids=["x".join(map(str, hid)) for hid, _ in NETS])
def test_host_driven_fp32_search_stays_inside_the_bound_and_the_share_cap(hid, E):
    """The cases of test_every_table_row_by_name_on_both_plans: (a) at six rounds, (b) at four."""
    for n in (20, 2):
        c = BT.case(hid, E, 37, n, BT.seed_of(hid, E))
        x6, x4 = _host_search(c, 6), _host_search(c, 4)
        for j in BT.JS:
            ratio = float(np.max(np.abs(x6[:, j] - c.xn[:, j]) / BT.truth_bound(c, j, BT.STEP6, TOL)))
            share, off_kept, off_left = _check_b(c, x4, j, 4)
            print(f"{list(hid)} n={n} j={j}: (a) {ratio:.3f} of the bound; (b) left out {100. * share:.1f} % ({off_left} differ), kept rows "
                  f"that differ {off_kept}")
            assert ratio <= 1. and share <= 0.10 and off_kept == 0


FAMILY_NETS = sorted({(tuple(hid), E) for _, _, hid, E in BT.FAMILIES})


@pytest.mark.parametrize("hid,E", FAMILY_NETS, ids=["x".join(map(str, hid)) for hid, _ in FAMILY_NETS])
def test_host_driven_fp32_search_at_one_and_ten_rounds(hid, E):
    c = BT.case(hid, E, 37, 20, BT.seed_of(hid, E))
    x1, x10 = _host_search(c, 1), _host_search(c, 10)
    for j in BT.JS:
        share, off_kept, _ = _check_b(c, x1, j, 1)
        ratio = float(np.max(np.abs(x10[:, j] - c.xn[:, j]) / BT.truth_bound(c, j, 0., TOL)))
        print(f"{list(hid)} j={j}: iters=1 left out {100. * share:.1f} %, iters=10 {ratio:.3f} of the bound")
        assert share <= 0.10 and off_kept == 0 and ratio <= 1.
