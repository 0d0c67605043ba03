"""The case table of tests/_bwd_coverage_cases.py, proved without a GPU: every case's hand-derived name is what
umnn_cc_backward_plan_name gives under the case's options; the cases cover every kernel name the plan header can produce (or the name
is in UNREACHED with the reason); every case's inputs keep the documented distance from the LeakyReLU kinks without rejecting more
than half of the draws; and the float64 truth wrapper agrees with the oracle the reference fixtures pin."""
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
