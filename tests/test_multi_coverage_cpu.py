"""The case table of tests/_multi_coverage_cases.py, proved without a GPU: the LDS arithmetic of multi_plan restated, every case's
family, pass list and waves per workgroup following from the restatement, umnn_cc_backward_multi_workspace_bytes agreeing with it at
the limits, all 10 forward and 12 backward instantiations of csrc/cc_multi.hip expected by some case, the kink guard within the
rejection cap, the extended truth pinned to tests/_multi_output_cases.py, the bound shown to bind, and the argument errors of the two
entries that tests/test_multi_output_cpu.py does not reach."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from tests import _multi_coverage_cases as C
from tests import _multi_output_cases as M
from tests import _util as U
from umnn_amd import _lib

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "umnn_amd", "csrc", "cc_multi.hip")


def _cus():
    """what umnn_num_cus answers in this process: the device's count, 256 without one"""
    return torch.cuda.get_device_properties(0).multi_processor_count if torch.cuda.is_available() else 256


def _large_cases(cus=256):
    a, b = C.large_shapes(cus)
    return [C.large_case(a), C.large_case(b)] + [C.large_case(a, fam, rep[0]) for fam, rep in C.REPS.items() if fam != (2, 8)]


# ---- the plan ---------------------------------------------------------------------------------------------------------------------
def test_lds_arithmetic_of_the_plan():
    assert [C.multi_ld(4 * ks) for _, ks in C.FAMILIES] == [46, 78, 78, 110, 142]
    assert C.LDS_FLOATS == 40960
    # (family, images, waves) -> floats, the figures of the case file's docstring
    for fam, nimg, waves, floats in (((2, 8), 6, 4, 6 * 1472 + 736 + 32 + 4 * 2304), ((4, 13), 5, 4, 39000), ((4, 13), 6, 4, 43056),
                                     ((4, 13), 6, 2, 34352), ((4, 16), 4, 4, 38688), ((4, 16), 5, 4, 43680), ((4, 16), 5, 2, 34976),
                                     ((7, 26), 2, 4, 40112), ((7, 26), 3, 4, 51552), ((7, 26), 3, 2, 43872), ((7, 26), 3, 1, 40032),
                                     ((8, 32), 1, 4, 37984), ((8, 32), 2, 1, 43104)):
        assert C.bwd_lds_floats(fam, nimg, waves) == floats, (fam, nimg, waves)
    assert 4 * C.bwd_lds_floats((7, 26), 3, 1) == 160128
    assert [C.wpb_of((2, 8), n) for n in range(7)] == [4] * 7
    assert [C.wpb_of((4, 13), n) for n in range(7)] == [4, 4, 4, 4, 4, 4, 2]
    assert [C.wpb_of((4, 16), n) for n in range(7)] == [4, 4, 4, 4, 4, 2, 2]
    assert [C.wpb_of((7, 26), n) for n in range(5)] == [4, 4, 4, 1, 0]
    assert [C.wpb_of((8, 32), n) for n in range(3)] == [4, 4, 0]
    # the cuts between the families, both sides
    for H, fam in ((15, (2, 8)), (16, (2, 8)), (31, (2, 8)), (32, (4, 13)), (51, (4, 13)), (52, (4, 16)), (63, (4, 16)), (64, (7, 26)),
                   (103, (7, 26)), (104, (8, 32)), (127, (8, 32))):
        assert C.family_of([H]) == fam and C.family_of([3, H, 7]) == fam, H


@pytest.mark.parametrize("c", C.CASES + _large_cases(), ids=lambda c: c["id"])
def test_table_follows_the_restated_rule(c):
    fam, nimg = C.family_of(c["hid"]), len(c["hid"]) - 1
    assert fam == c["fam"]
    assert c["fwd"] == C.fwd_name(*fam, 2 if c["part"] == 4 else 1)
    assert C.fwd_lds_floats(fam, nimg) <= C.LDS_FLOATS
    full, alone = C.passes_of(fam, nimg), C.passes_of(fam, nimg, need_theta=False)
    assert len(full) == c["passes"] and len(alone) == 1 and alone[0] == full[0]
    assert c["last"] == C.bwd_name(*fam, *full[-1]) and c["first"] == C.bwd_name(*fam, *full[0])
    assert C.wpb_of(fam, nimg) == c["wpb"]
    # exactly one pass holds the output layer's dW_L, every hidden image is held by exactly one pass, exactly one pass is the EDGE pass
    assert sum(o for _, _, o in full) == 1 and sum(e for _, e, _ in full) == 1 and full[0][1] == 1
    assert sum(n for n, _, _ in full) >= nimg


def test_part_1_reaches_every_depth_the_issue_names():
    depths = {}
    for c in C.CASES:
        if c["part"] == 1:
            depths.setdefault(c["fam"], set()).add(len(c["hid"]))
    assert depths[2, 8] >= {1, 3, 5, 6} and depths[4, 13] >= {1, 3, 5, 6, 7} and depths[4, 16] >= {1, 3, 5, 6}
    assert depths[7, 26] == {1, 2, 3, 4} and depths[8, 32] == {1, 2}
    assert {c["wpb"] for c in C.CASES} == {1, 2, 4}
    widths = {H for c in C.CASES if c["part"] == 1 for H in c["hid"]}
    assert widths >= {15, 16, 31, 32, 51, 52, 63, 64, 103, 104, 127}
    for fam in C.FAMILIES:
        assert {c["K"] for (f, _), c in C.FLAG_CASES.items() if f == fam} | {C.REP_CASES[fam]["K"]} == {2, 3, 4, 5, 13, 16}


def test_count_edges_reach_the_tile_and_workgroup_counts():
    tiles = {(c["B"], c["d"]): (c["B"] * c["d"] + 15) // 16 for c in C.COUNT_CASES}
    assert [c["B"] * c["d"] for c in C.COUNT_CASES] == [1, 15, 16, 17, 33, 129, 153, 315, 417, 501, 513]
    for shape, blocks in C.COUNT_BLOCKS.items():
        assert (tiles[shape] + 3) // 4 == blocks                     # forward workgroups of four waves, one tile each at P = 1
    assert (tiles[1, 1] + 3) // 4 == 1 and tiles[167, 3] == 32 and tiles[171, 3] == 33
    assert any(c["B"] * c["d"] % 16 and c["d"] > 16 for c in C.COUNT_CASES)      # a sample wider than a tile
    assert [c["n"] for c in C.NODE_CASES] == [1, 2, 3, 50] and [c["E"] for c in C.EMBED_CASES] == [0, 1, 5, 30]
    # shape A and B on a device of 256 CUs: P = 2 on an odd tile count, three groups on some waves, per = 65
    a, b = (C.large_case(s) for s in C.large_shapes(256))
    assert a["B"] == 32805 and (a["B"] + 15) // 16 == 2051 and 2051 > 2 * 1024 and a["B"] // 64 >= 512
    assert b["B"] * b["d"] == 65538 and -(-65538 // 1024) == 65 and -(-65538 // 65) == 1009


def test_every_instantiated_kernel_is_expected_by_a_case():
    src = open(CSRC).read()
    fwd = [C.fwd_name(*map(int, m)) for m in re.findall(r"MULTI_FWD\((\d+), (\d+), (\d+)\)", src)]
    bwd = [C.bwd_name(*map(int, m)) for m in re.findall(r"MULTI_BWD\((\d+), (\d+), (\d+), (\d+), (\d+)\)", src)]
    assert len(fwd) == 10 and len(set(fwd)) == 10 and len(bwd) == 12 and len(set(bwd)) == 12
    cases = C.CASES + _large_cases()
    assert {c["fwd"] for c in cases} == set(fwd)
    assert {c["last"] for c in cases} | {c["first"] for c in cases} == set(bwd)
    # every name but the seven-tile EDGE pass with a dW layer (always followed by another pass) is the LAST pass of some case
    assert set(bwd) - {c["last"] for c in cases} == {C.bwd_name(7, 26, 1, 1, 0)}


# ---- the workspace ----------------------------------------------------------------------------------------------------------------
def _ws(c, B, d=None):
    return _lib.lib().umnn_cc_backward_multi_workspace_bytes(ctypes.byref(C.desc(c)), B, c["d"] if d is None else d, c["E"])


@pytest.mark.parametrize("c", C.CASES + _large_cases(), ids=lambda c: c["id"])
def test_workspace_bytes_is_the_restated_sum(c):
    assert _ws(c, c["B"]) == C.workspace_bytes(c, c["B"] * c["d"], _cus())


def test_workspace_bytes_at_the_lds_limit_and_over_b():
    net = lambda hid: dict(hid=hid, K=5, E=4, d=3, act=C.LEAKY, out_act=C.ELU)
    lib = _lib.lib()
    assert _ws(net([103] * 4), 37) == C.workspace_bytes(net([103] * 4), 111, _cus()) > 0
    assert _ws(net([127, 104]), 37) == C.workspace_bytes(net([127, 104]), 111, _cus()) > 0
    assert _ws(net([127] * 3), 37) == -1 and lib.umnn_last_error() == b"multi-output backward: weight images exceed 160 KiB of LDS"
    # the forward's images themselves: five seven-tile layers, six eight-tile ones
    assert C.fwd_lds_floats((7, 26), 4) > C.LDS_FLOATS >= C.fwd_lds_floats((7, 26), 3)
    assert C.fwd_lds_floats((8, 32), 5) > C.LDS_FLOATS >= C.fwd_lds_floats((8, 32), 2)
    for hid in ([103] * 5, [127] * 6):
        assert _ws(net(hid), 37) == -1 and lib.umnn_last_error() == b"multi-output: weight images exceed 160 KiB of LDS"
    assert _ws(net([20, 20]), 37, d=0) == -1 and _ws(net([20, 20]), 0) == 0 and _ws(net([20, 20]), -3) == 0
    for c in (C.BY_ID["p1-20x31x9"], C.BY_ID["p1-103x4"]):
        sizes = [_ws(c, B) for B in (1, 5, 6, 21, 22, 341, 342, 21845, 21846, 21847, 30000, 1 << 20)]
        assert all(a > 0 for a in sizes) and sizes == sorted(sizes), sizes


# ---- inputs -----------------------------------------------------------------------------------------------------------------------
def _input_sets():
    seen, out = set(), []
    for c in C.CASES + _large_cases()[:2]:
        if C._input_key(c) not in seen:
            seen.add(C._input_key(c))
            out.append(c)
    return out


@pytest.mark.parametrize("c", _input_sets(), ids=lambda c: c["id"])
def test_inputs_stay_off_the_kinks_within_the_rejection_cap(c):
    i = C.inputs(c)
    print(f"{c['id']}: rejected {i.reject:.3f} of the rows drawn, smallest kept margin {i.margin:.2e}")
    assert i.reject <= C.REJECT_CAP and i.margin >= C.GUARD
    assert i.x.shape == (c["B"], c["d"]) and i.h.shape == (c["B"], c["E"] * c["d"]) and i.g.shape == (c["B"], c["d"], c["K"])
    assert (i.x0 is None) == (not c["x0"])
    x0 = torch.zeros_like(i.x) if i.x0 is None else i.x0
    assert C.margin_rows(i.net, x0.numpy(), i.x.numpy(), i.h.numpy(), c["n"]).min() >= C.GUARD
    assert torch.equal(i.x.float().double(), i.x) and torch.equal(i.h.float().double(), i.h) and torch.equal(i.g.float().double(), i.g)


# ---- truth and bounds -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("i,inv_f", [(0, False), (0, True), (1, False), (1, True), (2, False), (3, False), (4, False)])
def test_truth_is_the_truth_of_the_existing_cases(i, inv_f):
    """`quadrature` on the five cases of tests/_multi_output_cases.py (x [B, 1]: the rows are the samples; ELU with the + 1 outside)
    against its `case_truth`: 1e-12 of each tensor's largest entry."""
    import copy
    c = M.CASES[i]
    net, x, h, g = M.build(c)
    net64 = copy.deepcopy(net).double()
    got = C.quadrature(lambda rows: net64.net(rows) + 1.0, list(net64.parameters()), None, x[:, 0], h, g, c.nb_steps, inv_f)
    T = M.case_truth(i, inv_f)
    assert U.scaled_err(got.F, T.F) <= 1e-12 and U.scaled_err(got.dx, T.dx[:, 0]) <= 1e-12 and U.scaled_err(got.dh, T.dh) <= 1e-12
    assert len(got.dtheta) == len(T.dparams) and all(U.scaled_err(a, b) <= 1e-12 for a, b in zip(got.dtheta, T.dparams))
    assert U.scaled_err(got.fx, net64(x.double(), h.double()).detach().numpy()) <= 1e-12


def test_truth_of_dx0_d_and_sigmoid_against_a_second_derivation():
    """What `case_truth` does not have.  d = 3 with x0 and a sigmoid output: F row by row from IntegrandNetwork's own forward over
    [B, d] (its `rows` is the layout rule of h), d_x0 = -sum_k g_k f_k(x0), and d_h in the [B, E d] layout by autograd through that."""
    c = C.BY_ID["p2-20x31x9-sigmoid"]
    i, t = C.inputs(c), C.truth(c).t
    B, d, K, n = c["B"], c["d"], c["K"], c["n"]
    import copy
    net = copy.deepcopy(i.net)
    net.net = net.net.double()
    w, s = (v.reshape(-1).double() for v in C.compute_cc_weights(n))
    h = i.h.clone().requires_grad_()
    F = 0
    for j in range(n + 1):
        tj = i.x0 + (i.x - i.x0) * (s[j] + 1) / 2
        F = F + w[j] * net.net(net.rows(tj, h)).view(B, d, K)
    F = F * ((i.x - i.x0) / 2)[:, :, None]
    (F * i.g).sum().backward()
    assert U.scaled_err(t.F.reshape(B, d, K), F.detach().numpy()) <= 1e-12
    dh_rows = h.grad.view(B, c["E"], d).transpose(1, 2).reshape(B * d, c["E"])
    assert U.scaled_err(t.dh, dh_rows.numpy()) <= 1e-12
    with torch.no_grad():
        f0 = net.net(net.rows(i.x0, i.h)).view(B, d, K)
    assert U.scaled_err(t.dx0.reshape(B, d), -(f0 * i.g).sum(2).numpy()) <= 1e-12
    assert float(f0.max()) < 1.0 and float(f0.min()) > 0.0          # a sigmoid


@pytest.mark.parametrize("id", ["p1-20x31x9", "p1-103x4", "p2-127x104-inv_f", "p3-E0", "p3-count-5x63"])
def test_the_bound_binds(id):
    """The float32 run itself meets the bound (it is within E32 <= M E32); moved by 16 x E32 it does not -- for every output."""
    c = C.BY_ID[id]
    T = C.truth(c)
    e = C.errors(T.t32, T.t)
    for name in C.VALUES + C.GRADS:
        if name == "dh" and c["E"] == 0:
            continue
        tensors = zip(T.t32.dtheta, T.t.dtheta, T.E32["dtheta"], e["dtheta"]) if name == "dtheta" else \
            [(getattr(T.t32, name), getattr(T.t, name), T.E32[name], e[name])]
        for a32, a64, E32, err in tensors:
            b = C.bound(E32, name)
            assert C.FLOOR <= E32 and 8 * C.FLOOR <= b <= M.TOL and err <= E32 < b
            scale = np.maximum(np.abs(a64), 1.0) if name in C.VALUES + ("dx0", "dx") else np.abs(a64).max()
            moved = a32 + 16 * E32 * scale
            crit = U.rel_err if name in C.VALUES + ("dx0", "dx") else U.scaled_err
            assert crit(moved, a64) > b, (id, name)


# ---- argument errors --------------------------------------------------------------------------------------------------------------
def test_argument_errors_of_the_two_entries():
    lib = _lib.lib()
    p = ctypes.c_void_p(0x1000)
    c = C.BY_ID["p1-20x31x9"]
    m = C.desc(c)
    B, d, E = 4, 3, c["E"]
    need = _ws(c, B)
    assert need > 0

    def bwd(desc=m, n=6, B=B, d=d, ws=p, nbytes=need):
        return lib.umnn_cc_backward_multi(ctypes.byref(desc), None, p, p, p, p, p, n, B, d, E, 0, None, None, None, None, ws, nbytes, None)

    def fwd(desc=m, n=6, B=B, d=d):
        return lib.umnn_cc_forward_multi(ctypes.byref(desc), None, p, p, p, p, n, B, d, E, 0, p, None, None, None)

    assert bwd(nbytes=need - 1) == _lib.EINVAL and b"workspace smaller" in lib.umnn_last_error()
    assert bwd(ws=None) == _lib.EINVAL and b"workspace smaller" in lib.umnn_last_error()
    assert bwd(nbytes=0) == _lib.EINVAL and b"workspace smaller" in lib.umnn_last_error()
    for n in (0, -1):
        assert bwd(n=n) == _lib.EINVAL and b"nb_steps" in lib.umnn_last_error()
        assert fwd(n=n) == _lib.EINVAL and b"nb_steps" in lib.umnn_last_error()
        assert fwd(n=n, B=0) == _lib.EINVAL                       # (the empty batch does not hide it)
    for bad in (0, -2):
        assert bwd(d=bad) == _lib.EINVAL and b"d >= 1" in lib.umnn_last_error()
        assert fwd(d=bad) == _lib.EINVAL and b"d >= 1" in lib.umnn_last_error()
    assert bwd(B=-1) == _lib.EINVAL and fwd(B=-1) == _lib.EINVAL
    for K in (1, 17):
        k = C.desc(dict(c, K=K))
        assert fwd(desc=k) == _lib.EINVAL and b"output width" in lib.umnn_last_error()
        assert bwd(desc=k) == _lib.EINVAL and b"output width" in lib.umnn_last_error()
        assert lib.umnn_cc_backward_multi_workspace_bytes(ctypes.byref(k), B, d, E) == -1
    # a net the backward has no room for is refused by the backward entry too, before it looks at the workspace; the forward plans it
    deep = C.desc(dict(c, hid=[127] * 3))
    assert bwd(desc=deep) == _lib.EUNSUPPORTED and b"backward: weight images exceed" in lib.umnn_last_error()
    assert fwd(desc=deep, B=0) == 0
    assert bwd(B=0, ws=None, nbytes=0) == 0                          # (B = 0 without d_theta: nothing to do, no workspace needed)
