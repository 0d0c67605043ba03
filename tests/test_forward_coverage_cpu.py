"""The case table of tests/_fwd_coverage_cases.py, proved without a GPU: every case's hand-derived name, P, ns, waves, pieces and
fallback are what umnn_cc_launch_plan gives under the case's options; the cases name every forward kernel csrc/cc_fwd_plan.h
instantiates (or the name is in UNREACHED with the reason); the float64 truth agrees with the oracle the reference fixtures pin; and
every case's E32 is small enough that M x E32, not the outer 1e-4, is the bound that binds."""
import ctypes

import numpy as np
import pytest

from oracle import cc_oracle as O
from tests import _fwd_coverage_cases as C
from umnn_amd import _lib


def _plan(c, flags=None):
    info = _lib.LaunchPlanInfo()
    with _lib.options(**c["options"]):
        rc = _lib.lib().umnn_cc_launch_plan(ctypes.byref(C.mlp_desc(c)), _lib.PLAN_FORWARD, c["B"], c["d"], c["E"], c["n"],
                                            C.plan_flags(c) if flags is None else flags, ctypes.byref(info))
    return rc, info


@pytest.mark.parametrize("c", C.CASES, ids=[c["id"] for c in C.CASES])
def test_plan(c):
    rc, info = _plan(c)
    assert rc == 0
    got = (info.name.decode(), info.pieces, info.P, info.ns, info.waves_per_block, info.fallback)
    assert got == (c["name"], c["pieces"], c["P"], c["ns"], c["waves"], c["fallback"])
    groups = -(-c["B"] * c["d"] // (32 if c["name"] == C.P32 else 16 * c["P"]))
    assert info.blocks == -(-groups // (c["waves"] // c["ns"]))


# ---- completeness: the 81 names by their generating rule (cc_fwd_plan.h) ------------------------------------------------------------
# UMNN_FWD_ROWS_2 / _WIDE_FIRST / _3: (T, NPARTS, P, EXACT, LIVE, PIPE, TREST, WPB)
ROWS_2 = [(4, 2, 2, 1, 13, 1, 0, 4), (4, 2, 2, 1, 0, 1, 0, 4), (4, 2, 1, 1, 13, 0, 0, 4), (4, 2, 2, 1, 13, 0, 0, 4), (4, 2, 1, 1, 0, 0, 0, 4),
          (4, 2, 2, 1, 0, 0, 0, 4), (2, 2, 1, 0, 0, 0, 0, 4), (2, 2, 2, 0, 0, 0, 0, 4), (4, 2, 1, 0, 0, 0, 0, 4), (4, 2, 2, 0, 0, 0, 0, 4),
          (7, 2, 1, 1, 26, 0, 0, 4), (7, 2, 1, 1, 0, 0, 0, 4), (5, 2, 1, 1, 0, 0, 0, 4), (6, 2, 1, 1, 0, 0, 0, 4), (8, 2, 1, 1, 0, 0, 0, 4),
          (7, 2, 1, 1, 26, 0, 0, 8), (7, 2, 1, 1, 0, 0, 0, 8), (5, 2, 1, 1, 0, 0, 0, 8), (6, 2, 1, 1, 0, 0, 0, 8), (8, 2, 1, 1, 0, 0, 0, 8),
          (8, 2, 1, 0, 0, 0, 0, 4), (8, 2, 2, 0, 0, 0, 0, 4)]
ROWS_WIDE_FIRST = [(t1, 2, 1, 1, live, 0, 4, 4) for live in (13, 0) for t1 in (5, 6, 7, 8)]
ROWS_3 = [(4, 3, 1, 1, 13, 0, 0, 4), (4, 3, 2, 1, 13, 0, 0, 4), (4, 3, 1, 1, 0, 0, 0, 4), (4, 3, 2, 1, 0, 0, 0, 4), (2, 3, 1, 0, 0, 0, 0, 4),
          (2, 3, 2, 0, 0, 0, 0, 4), (4, 3, 1, 0, 0, 0, 0, 4), (4, 3, 2, 0, 0, 0, 0, 4)]
# UMNN_FWD_FP32_VARIANTS: (T, KS, P, TAIL)
FP32_VARIANTS = [(4, 13, 1, 1), (4, 13, 2, 1), (4, 13, 1, 0), (4, 13, 2, 0), (7, 26, 1, 0), (7, 26, 2, 0), (2, 0, 1, 0), (2, 0, 2, 0), (4, 0, 1, 0),
                 (4, 0, 2, 0), (8, 0, 1, 0), (8, 0, 2, 0)]
UNREACHED = {}      # name: reason.  Empty: every instantiated forward kernel is the name of a case.


def _row_name(stem, T, NP, P, EX, NR, PIPE, TREST, WPB):
    if TREST:
        return f"{stem}<T1={T},TREST={TREST},PARTS={NP},P={P},EXACT={EX},LIVE={NR}>"
    return f"{stem}<T={T},PARTS={NP},P={P},EXACT={EX},LIVE={NR}{',PIPE' if PIPE else ''}{',WAVES=8' if WPB == 8 else ''}>"


def _all_names():
    names = [_row_name("cc_fwd_f16", *r) for r in ROWS_2 + ROWS_WIDE_FIRST]
    names += [_row_name("cc_fwd_bf16", *r) for r in ROWS_2 + ROWS_WIDE_FIRST + ROWS_3]
    names += [f"cc_fwd<T={t},KS={k},P={p},TAIL={tl}>" for t, k, p, tl in FP32_VARIANTS]
    return names + [C.P32]


def test_every_kernel_name_is_the_name_of_a_case_or_explained():
    names = _all_names()
    assert len(names) == 30 + 30 + 8 + 12 + 1 == 81 and len(set(names)) == 81
    covered = {c["name"] for c in C.CASES}
    assert covered <= set(names), covered - set(names)
    for name in names:
        assert (name in covered) != (name in UNREACHED), name
    # ... and part 1 runs each of them with the node range whole and split
    part1 = {}
    for c in C.CASES:
        if c["part"] == 1:
            part1.setdefault(c["name"], set()).add(c["ns"])
    assert set(part1) == set(names) - set(UNREACHED)
    assert all(ns == ({1} if name == C.P32 else {1, 4}) for name, ns in part1.items())


def test_the_plan_names_only_instantiated_kernels_and_none_that_is_unreached():
    """A sweep over nets (equal, mixed, wide-first, narrow, one hidden layer), batch sizes, node counts and options: whatever the plan
    names is one of the 81, and never an UNREACHED one."""
    names, seen = set(_all_names()), set()
    nets = [[50] * 4, [60] * 4, [48, 60, 36, 50], [20, 20], [20, 40], [50], [100], [100, 100], [100] * 3, [110] * 3, [70] * 5, [90] * 4, [120] * 3,
            [70, 90], [120, 20, 20], [63, 64], [31, 31, 31], [127] * 2] + [[w1] + rest for w1 in (70, 90, 100, 120) for rest in ([50, 50], [60, 60], [20] * 4)]
    opts = [dict(), dict(fwd_p=2), dict(fwd_p=2, fwd_pipe=0), dict(fwd_pad=0), dict(fwd_pad_min=4), dict(fwd_tail=0), dict(fwd_pipe=2), dict(fwd_ns=2)]
    for hid in nets:
        for prec in _lib.PRECISIONS.values():
            for o in opts:
                for B, n, flags in ((37, 20, 0), (37, 2, 0), (40000, 20, 0), (37, 20, _lib.PLAN_MARKER_ALIASED)):
                    c = dict(hid=hid, E=4, B=B, d=3, n=n, act=C.LEAKY, out_act=C.ELU, options=dict(fwd_precision=prec, **o))
                    rc, info = _plan(c, flags)
                    assert rc == 0 and info.name.decode() in names and info.name.decode() not in UNREACHED, (hid, o, info.name)
                    assert 1 <= info.ns <= n + 1
                    seen.add(info.name.decode())
    assert len(seen) > 60      # (the sweep itself reaches most of the table)


# ---- the truth ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("id", ["rep-f16-exact13", "rep-f16-exact13-no-x0", "rep-f16-wide-first-inv_f", "rep-fp32-generic-sigmoid", "rep-bf16-2-relu"])
def test_truth_is_the_pinned_oracle(id, monkeypatch):
    """quadrature64 (torch, float64, the module's own forward) against oracle.integrate_parallel / integrand (numpy float64, pinned by
    the reference's fixtures): 1e-12.  The oracle's float64 mode builds float64 tables (2e-8 from the float32-rounded ones the kernels
    read), so it is handed the rounded ones: the same quadrature, two derivations."""
    monkeypatch.setattr(O, "cc_tables", lambda n, dtype=np.float32: C.cc_tables_rounded(n, dtype))
    c = C.BY_ID[id]
    i, r = C.inputs(c), C.reference(c)
    net = C.oracle_net(i.net, np.float64)
    x, h = i.x.double().numpy(), i.h.double().numpy()
    x0 = i.x0.double().numpy() if c["x0"] else np.zeros_like(x)
    for got, ref in ((r.F, O.integrate_parallel(net, x0, x, h, c["n"], inv_f=c["inv_f"])), (r.fx, O.integrand(net, x, h)), (r.fx0, O.integrand(net, x0, h))):
        assert ref.dtype == np.float64 and np.abs(got - ref).max() <= 1e-12 * max(1.0, np.abs(ref).max())


def _reference_sets():
    seen, out = set(), []
    for c in C.CASES:
        key = C._input_key(c) + (c["n"], c["x0"], c["inv_f"])
        if key not in seen:
            seen.add(key)
            out.append(c)
    return out


def test_the_tight_bound_is_the_one_that_binds():
    """E32 of every distinct (input set, n, x0, inv_f) is finite and below 1e-5 on all three outputs, so 8 x E32 and 64 x E32 stay under
    the outer 1e-4 ... for the fp32-level modes always, for bf16x3 while E32 < 1.56e-6 (asserted per case: min() never picks 1e-4)."""
    worst = 0.0
    for c in _reference_sets():
        r = C.reference(c)
        assert all(np.isfinite(e) and e < 1e-5 for e in r.E32), (c["id"], r.e32)
        assert all(np.isfinite(t).all() for t in (r.F, r.fx, r.fx0))
        worst = max(worst, *r.e32)
    for c in C.CASES:
        assert all(b < C.OUTER for b in C.bounds(c)), (c["id"], C.bounds(c))
    # block 2 of the log-likelihood chain reads another x (chain_x2): its reference is no case's, so it is held to the same here
    for c in C.LL_CASES:
        r2 = C.ll_reference(c).r2.ref
        assert all(np.isfinite(e) and e < 1e-5 and C.M(c) * e < C.OUTER for e in r2.E32), (c["id"], r2.e32)
        worst = max(worst, *r2.e32)
    print(f"largest e32 of any case {worst:.2e}")


def test_bf16_storage_inputs_hold_bf16_values():
    import torch
    c = C.BY_ID["rep-f16-exact13-xh-bf16"]
    i = C.inputs(c)
    assert all(torch.equal(t.to(torch.bfloat16).float(), t) for t in (i.x, i.x0, i.h, i.lj_in))
    assert not torch.equal(C.inputs(C.BY_ID["rep-f16-exact13"]).x.to(torch.bfloat16).float(), C.inputs(C.BY_ID["rep-f16-exact13"]).x)


def test_the_chain_truth_is_the_oracles_compute_ll(monkeypatch):
    """ll_reference against oracle.flow_compute_ll's arithmetic restated on two blocks with the same embedding: block_log_jac and the
    Gaussian term in numpy float64 on the rounded tables, 1e-12."""
    monkeypatch.setattr(O, "cc_tables", lambda n, dtype=np.float32: C.cc_tables_rounded(n, dtype))
    c = C.BY_ID["ll-f16-exact13-9x17-nsauto"]
    i, r = C.inputs(c), C.ll_reference(c)
    net = C.oracle_net(i.net, np.float64)
    h, s = i.h.double().numpy(), i.scaling.double().numpy()
    ll = 0.0
    for x in (i.x.double().numpy(), C.chain_x2(c).double().numpy()):
        z = np.exp(s)[None, :] * (O.integrate_parallel(net, np.zeros_like(x), x, h, c["n"]) + h[:, :c["d"]])
        ll = ll + (np.log(O.integrand(net, x, h) + 1e-10) + s[None, :]).sum(1)
    ll = ll - 0.5 * (np.log(2 * np.pi) + z ** 2).sum(1)
    assert np.abs(r.ll - ll).max() <= 1e-12 * max(1.0, np.abs(ll).max())
    assert (r.bll > 0).all() and (r.bll < 1e-3).all()
