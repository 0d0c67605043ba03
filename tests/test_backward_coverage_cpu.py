"""The case table of tests/_bwd_coverage_cases.py, proved without a GPU: every case's hand-derived name is what
umnn_cc_backward_plan_name gives under the case's options; the cases cover every kernel name the plan header can produce (or the name
is in UNREACHED with the reason); every case's inputs keep the documented distance from the LeakyReLU kinks without rejecting more
than half of the draws; the float64 truth wrapper agrees with the oracle the reference fixtures pin; every case has an arithmetic class
by the stated rule; and the bounds built on the yardsticks reject a wrong LeakyReLU slope that the flat tolerance lets through."""
import ctypes

import numpy as np
import pytest
import torch

from oracle import cc_oracle as O
from tests import _bwd_coverage_cases as C
from umnn_amd import _lib


def _plan_name(c):
    m = C.desc(c)
    with _lib.options(**c["options"]):
        return _lib.lib().umnn_cc_backward_plan_name(ctypes.byref(m), c["B"], c["d"], c["E"], c["n"], C.plan_flags(c)).decode()


@pytest.mark.parametrize("c", C.CASES, ids=[c["id"] for c in C.CASES])
def test_plan_name(c):
    assert _plan_name(c) == c["name"]


def test_nets_without_a_kernel_are_errors():
    for hid in C.NO_KERNEL:
        c = dict(hid=hid, E=4, act=C.LEAKY, out_act=C.ELU)
        for precision in (C.FP32, _lib.PRECISIONS["bf16x3"]):
            with _lib.options(bwd_precision=precision):
                assert _lib.lib().umnn_cc_backward_plan_name(ctypes.byref(C.desc(c)), 9, 3, 4, 6, 0) == b""


# kBwdKernelNames by its generating rule (cc_bwd_plan.h): eight kinds x UMNN_BWD_LOOP_SHAPES / UMNN_BWD_WS_SHAPES
LOOP_SHAPES = [(4, 13), (3, 13), (2, 13), (4, 0), (3, 0), (2, 0)]
WS_SHAPES = [(4, 13), (4, 0)]
KINDS = [(LOOP_SHAPES, "cc_bwd_bf16", ",EDGE=1,", ""), (LOOP_SHAPES, "cc_bwd_bf16", ",", ",SWP"), (WS_SHAPES, "cc_bwd_bf16", ",", ",WS"),
         (WS_SHAPES, "cc_bwd_f16", ",", ",WS"), (LOOP_SHAPES, "cc_bwd_bf16", ",EDGE=1,", ",FRONT"), (LOOP_SHAPES, "cc_bwd_bf16x6", ",EDGE=1,", ",FRONT"),
         (WS_SHAPES, "cc_bwd_bf16", ",", ",WS,FRONT"), (WS_SHAPES, "cc_bwd_f16", ",", ",WS,FRONT")]
# UMNN_BWD_FP32_VARIANTS: (T, NACC, EDGE, KS)
FP32_VARIANTS = [(4, 3, 1, 13), (4, 3, 0, 13), (2, 3, 1, 0), (2, 3, 0, 0), (4, 3, 1, 0), (4, 3, 0, 0), (5, 2, 1, 17), (5, 3, 0, 17), (7, 1, 1, 26),
                 (7, 0, 1, 26), (7, 1, 0, 26), (7, 0, 1, 0), (7, 1, 0, 0), (8, 0, 1, 0), (8, 1, 0, 0), (8, 0, 1, 32), (8, 1, 0, 32)]
UNREACHED = {
    # best_nacc(7, 1, 26) walks NACC = 3..0 and stops at the first instantiated EDGE=1 variant of the (7, 26) family, which is NACC=1;
    # the route asks find_bwd for exactly that NACC, and pick_tmax_bwd / pad_to_exact_family only ever hand (7, 26) to the exact
    # family, never to a generic one.  Confirmed by test_the_unreached_variant_is_never_named below.
    "cc_bwd<T=7,NACC=0,EDGE=1,KS=26>": "best_nacc prefers NACC=1 for (T=7, EDGE=1, KS=26); nothing else selects a variant",
}


def _all_names():
    names = [f"{stem}<L={lh}{middle}LIVE={nr}{tail}>" for shapes, stem, middle, tail in KINDS for lh, nr in shapes]
    return names + [f"cc_bwd<T={t},NACC={n},EDGE={e},KS={k}>" for t, n, e, k in FP32_VARIANTS]


def test_every_kernel_name_is_the_name_of_a_case_or_explained():
    names = _all_names()
    assert len(names) == 32 + 17 and len(set(names)) == len(names)
    covered = {c["name"] for c in C.CASES} | {a for c in C.CASES for a in c["also"]}
    assert covered <= set(names), covered - set(names)
    for name in names:
        assert (name in covered) != (name in UNREACHED), name
    # a first pass listed under `also` is one that holds no dW layer (NACC=0, EDGE=1): a pass with dW follows it in every call
    assert all("NACC=0,EDGE=1" in a for c in C.CASES for a in c["also"])


def test_the_unreached_variant_is_never_named():
    """No net of two to six equal or unequal hidden widths 97..103 (seven tiles, 26 K-steps, alone or after zero-padding) is routed
    to a pass whose last kernel is the NACC=0 variant, in either precision."""
    for precision in (C.FP32, _lib.PRECISIONS["bf16x3"]):
        for hid in ([100] * 2, [100] * 3, [100] * 4, [97, 103], [100, 80, 70], [70, 90], [103] * 6):
            c = dict(hid=hid, E=4, act=C.LEAKY, out_act=C.ELU)
            with _lib.options(bwd_precision=precision):
                assert _lib.lib().umnn_cc_backward_plan_name(ctypes.byref(C.desc(c)), 9, 3, 4, 6, 0).decode() not in UNREACHED


def test_every_front_variant_runs_in_every_build_and_stage_c():
    """kFrontVariants (cc_backward_front.hip): T1 = 5..8 x NL2 = 13, 0.  The two-piece build runs stage C as front_bwd2 says (0: bwd,
    1: bwd2, or bwd16 behind the fp16 middle stage, 2: bwd2 also there); the three-piece build has one stage C."""
    seen = set()
    for c in C.CASES:
        if not c["family"].startswith("FRONT"):
            continue
        t1, nl2 = (c["hid"][0] + 16) // 16, (13 if (c["hid"][1] + 4) // 4 == 13 else 0)
        if c["options"].get("bwd_precision") == C.FP32:
            seen.add((t1, nl2, 3, None))
            continue
        b2 = c["options"].get("front_bwd2", 1)
        seen.add((t1, nl2, 2, b2))
        if c["name"].startswith("cc_bwd_f16"):
            seen.add((t1, nl2, 2, {0: "bwd behind fp16", 1: "bwd16", 2: "bwd2 behind fp16"}[b2]))
    want = {(t1, nl2, 2, s) for t1 in (5, 6, 7, 8) for nl2 in (13, 0) for s in (0, 1, 2, "bwd16", "bwd2 behind fp16")}
    want |= {(t1, nl2, 3, None) for t1 in (5, 6, 7, 8) for nl2 in (13, 0)}
    assert want <= seen, sorted(want - seen, key=str)


def _input_sets():
    seen, out = set(), []
    for c in C.CASES:
        key = C._input_key(c)
        if key not in seen:
            seen.add(key)
            out.append(c)
    return out


@pytest.mark.parametrize("c", _input_sets(), ids=[c["id"] for c in _input_sets()])
def test_inputs_stay_off_the_kinks_within_the_rejection_cap(c):
    assert c["guard"] == C.GUARD or (c["guard"] == C.LOW_GUARD and c["n"] >= 255 and c["d"] == 1), "only the long quadratures lower the guard"
    i = C.inputs(c)
    print(f"{c['id']}: rejected {i.reject:.3f} of the rows drawn, smallest kept margin {i.margin:.2e}")
    assert i.reject <= C.REJECT_CAP
    assert i.margin >= c["guard"]
    assert i.x.shape == (c["B"], c["d"]) and i.h.shape == (c["B"], c["E"] * c["d"])
    # the margin of the kept rows, recomputed on the returned tensors
    x0 = torch.zeros_like(i.x) if i.x0 is None else i.x0
    assert C.margin_rows(i.net, x0.numpy(), i.x.numpy(), i.h.numpy(), c["n"]).min() >= c["guard"]
    # values of the storage type
    xdt = torch.bfloat16 if c["x_bf16"] else torch.float32
    hdt = torch.bfloat16 if c["h_bf16"] else torch.float32
    assert torch.equal(i.x.to(xdt).double(), i.x) and torch.equal(i.h.to(hdt).double(), i.h) and torch.equal(i.g.to(xdt).double(), i.g)


@pytest.mark.parametrize("id", ["rep-SWP", "rep-SWP-inv_f", "rep-FRONT-no-g_fx"])
def test_truth_is_the_pinned_oracle(id, monkeypatch):
    """tests/_truth64.backward_reference (torch autograd, float64) against oracle.integrate_backward + integrand_vjp (manual backprop in
    numpy float64, pinned by the reference's own fixtures): 1e-12 of each tensor's largest entry.  The evaluator integrates, like the
    kernels and the reference, with the float32-rounded Clenshaw-Curtis tables of compute_cc_weights; the oracle's float64 mode builds
    float64 tables (2e-8 apart, tests/test_gpu_round5.py), so it is handed the rounded ones here: same quadrature, two derivations."""
    from umnn_amd.quadrature import compute_cc_weights
    monkeypatch.setattr(O, "cc_tables", lambda n, dtype=np.float32: tuple(t.reshape(-1).numpy().astype(dtype) for t in compute_cc_weights(n)))
    c = C.BY_ID[id]
    i = C.inputs(c)
    lins = [m for m in i.net.net if isinstance(m, torch.nn.Linear)]
    onet = O.Net([l.weight.detach().double().numpy() for l in lins], [l.bias.detach().double().numpy() for l in lins], O.LEAKY, O.ELU1)
    x0, x, h, g = (t.numpy() for t in (i.x0, i.x, i.h, i.g))
    rdx0, rdx, rdh, _, _, rflat = O.integrate_backward(onet, x0, x, h, c["n"], g, inv_f=c["inv_f"])
    if i.g_fx is not None:
        jdx, jdh, jflat = O.integrand_vjp(onet, x, h, i.g_fx.numpy())
        rdx, rdh, rflat = rdx + jdx, rdh + jdh, rflat + jflat
    for got, ref in zip(C.truth(c), (rdx0, rdx, rdh, rflat)):
        assert np.abs(got.numpy() - ref).max() <= 1e-12 * np.abs(ref).max()


# ---- arithmetic classes, yardsticks and the bounds built from them ------------------------------------------------------------------
@pytest.mark.parametrize("c", C.CASES, ids=[c["id"] for c in C.CASES])
def test_every_case_has_a_class_by_the_stated_rule(c):
    """d_x0 and d_x are class A everywhere; d_h and d_theta are class B exactly for cc_bwd_bf16<...> and for the fp16 middle stage
    whose stage C runs on bf16 pieces (cc_bwd_plan.h: every front_bwd2 but 1), class A for cc_bwd<...>, cc_bwd_f16<...> otherwise and
    cc_bwd_bf16x6<...>; the emulated two-piece layers are the hidden-to-hidden ones of exactly the class B cases."""
    cls = C.arith_class(c)
    assert set(cls) == set(C.OUTPUTS) and set(cls.values()) <= {"A", "B"}
    assert cls["d_x0"] == cls["d_x"] == "A" and cls["d_h"] == cls["d_theta"]
    stem = c["name"].split("<")[0]
    assert stem in ("cc_bwd", "cc_bwd_f16", "cc_bwd_bf16", "cc_bwd_bf16x6")
    b = stem == "cc_bwd_bf16" or (stem == "cc_bwd_f16" and c["name"].endswith(",FRONT>") and c["options"].get("front_bwd2", 1) in (0, 2))
    assert cls["d_h"] == ("B" if b else "A")
    n_hidden = len(c["hid"])
    assert C.split_layers(c) == (() if not b else tuple(range(1, n_hidden)) if stem == "cc_bwd_bf16" else (1,))
    assert C.bound_of("d_x0") == C.bound_of("d_x") == C.bound_of("d_h") == C.bound_of("d_theta") == C.M_GRAD and set(C.M_OF) == {"d_theta:b_out"}


def test_both_classes_and_every_two_piece_form_are_present():
    stems = {(c["name"].split("<")[0], c["family"], C.arith_class(c)["d_h"]) for c in C.CASES}
    for fam in ("LOOP", "SWP", "WS", "FRONT", "FRONT_WS"):
        assert ("cc_bwd_bf16", fam, "B") in stems
    assert ("cc_bwd_f16", "FRONT_WS16", "B") in stems and ("cc_bwd_f16", "FRONT_WS16", "A") in stems and ("cc_bwd_f16", "WS16", "A") in stems
    assert ("cc_bwd_bf16", "WS16", "B") in stems and ("cc_bwd_bf16", "FRONT_WS16", "B") in stems        # (the fp16 pipeline not eligible)
    assert ("cc_bwd_bf16x6", "FRONT_P3", "A") in stems and ("cc_bwd", "FP32", "A") in stems


def test_two_piece_emulation_changes_only_the_backward_of_the_named_layers():
    """The emulated net's forward is exact: d_x0 = -f(x0) g is the truth's to the bit.  (Its d_x is not looked at: autograd takes the
    g_fx tangent back through the split W^T products, where the kernels take it forward through the recompute -- class A.)  d_h and
    d_theta move by the three-term figure, 1e-6 .. 3e-5, every parameter tensor by less than the flat tolerance."""
    c = C.BY_ID["rep-SWP"]
    y, ref = C.yardsticks(c), C.truth(c)
    assert C.split_layers(c) == (1, 2, 3)
    i = C.inputs(c)
    got = C._truth64.backward_reference(C.three_term_net(c), i.x0, i.x, i.h, i.g, i.g_fx, c["n"], chunk=1024)
    assert torch.equal(got[0], ref[0])
    for nm in ("d_h", "d_theta"):
        assert 1e-6 < y["E3"][nm] < 3e-5, (nm, y["E3"][nm])
    assert all(C.FLOOR <= e < 1e-4 for e in y["E3"]["tensors"])
    assert len(y["tensors"]) == 2 * (len(c["hid"]) + 1) == len(C.param_sizes(c)) and sum(C.param_sizes(c)) == ref[3].numel()


@pytest.mark.parametrize("key", [k for k in C.Z2_CASES if len(k) == 4], ids=lambda k: f"{k[0]}-NL2={k[1]}")
def test_saved_z2_cases_with_a_bf16_embedding(key):
    """T1 = 5 and 8, NL2 = 13 and 0, with g_fx: the three-stage name under PLAN_H_BF16, the library offers the pair, and the inputs (bf16
    values of h) keep their kink margin within the rejection cap."""
    c = C.Z2_CASES[key]
    assert c["h_bf16"] and not c["x_bf16"] and c["g_fx"] and not c["x0"] and key[3] == "h-bf16"
    assert (C.FRONT_W1[key[0]], 13 if (c["hid"][1] + 4) // 4 == 13 else 0) == ({70: 5, 120: 8}[key[0]], key[1])
    assert _plan_name(c) == c["name"] == f"cc_bwd_bf16<L=2,EDGE=1,LIVE={key[1]},FRONT>"
    assert _lib.lib().umnn_cc_forward_z2_floats(ctypes.byref(C.desc(c)), c["B"], c["d"], c["E"], c["n"]) > 0
    i = C.inputs(c)
    assert i.reject <= C.REJECT_CAP < 1 and i.margin >= C.GUARD
    assert torch.equal(i.h.to(torch.bfloat16).double(), i.h)
    assert C.arith_class(c)["d_h"] == "B"


def test_the_bf16_embedding_pair_covers_both_ends_of_t1_and_both_nl2():
    assert sorted(k[:2] for k in C.Z2_CASES if len(k) == 4) == [(70, 0), (70, 13), (120, 0), (120, 13)]


def _wrong_slope_run(c, slope):
    """the reference's own float32 arithmetic on a net whose LeakyReLU slope is `slope`"""
    import copy
    i = C.inputs(c)
    net = copy.deepcopy(i.net)
    for k, m in enumerate(net.net):
        if isinstance(m, torch.nn.LeakyReLU):
            net.net[k] = torch.nn.LeakyReLU(slope)
    return C._truth64.backward_reference(net, i.x0, i.x, i.h, i.g, i.g_fx, c["n"], dtype=torch.float32, chunk=1024)


@pytest.mark.parametrize("id", ["rep-FP32", "fp32-100x2", "ws16-60x60x60x60"])
def test_the_bounds_bind_where_the_flat_tolerance_does_not(id):
    """One class A case per family group.  A LeakyReLU slope of 0.01001 instead of 0.01 in the reference's float32 run -- an arithmetic
    error of an fp32-level kernel -- passes the flat TOL = 1e-4 in all four outputs and fails M_GRAD x E32 in all four; the unchanged
    float32 run passes both (it defines E32: ratio at most 1)."""
    c = C.BY_ID[id]
    assert set(C.arith_class(c).values()) == {"A"}
    ref, y = C.truth(c), C.yardsticks(c)
    wrong = C.errors(c, _wrong_slope_run(c, 0.01001), ref)
    right = C.errors(c, _wrong_slope_run(c, 0.01), ref)
    for nm in C.OUTPUTS:
        print(f"{id} {nm}: slope 0.01001 error {wrong[nm]:.2e} = {wrong[nm] / y[nm]:.0f} x E32 {y[nm]:.2e}")
        assert wrong[nm] < C.TOL
        assert wrong[nm] > C.M_GRAD * y[nm]
        assert right[nm] <= y[nm]
    assert any(a > C.M_GRAD * b for a, b in zip(wrong["tensors"], y["tensors"]))
    with pytest.raises(AssertionError):
        C.check_bounds(c, _wrong_slope_run(c, 0.01001), ref)
    C.check_bounds(c, _wrong_slope_run(c, 0.01), ref)


def test_flat_yardsticks_stay_below_the_flat_tolerance():
    """Over every input set: M_GRAD x the flat yardstick of every output is below TOL, so the new bounds are the tighter ones everywhere
    (class A: at most 8 x 3.2e-6; class B: at most 8 x 1.2e-5).  Per parameter tensor nothing is capped: a one-element output bias that
    is a cancelling sum carries its own float32 error."""
    worst, n_b, over = {}, 0, 0
    for c in C.CASES:
        y, cls = C.yardsticks(c), C.arith_class(c)
        for nm in C.OUTPUTS:
            worst[cls[nm], nm] = max(worst.get((cls[nm], nm), 0.0), y[nm])
            assert C.FLOOR <= y[nm] and C.M_GRAD * y[nm] < C.TOL, (c["id"], nm, y[nm])
        if cls["d_h"] == "B":
            n_b += 2
            over += sum(C.M_GRAD * y["E3"][nm] > C.TOL for nm in ("d_h", "d_theta"))
    print({k: f"{v:.2e}" for k, v in worst.items()}, f"class B outputs: {n_b}, with 8 x E3 above TOL: {over}")
    assert n_b > 0 and over == 0
