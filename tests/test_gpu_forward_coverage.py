"""The quadrature forward on every kernel variant, launch plan, flag and entry point, at the smallest shapes at which each runs: the
cases of tests/_fwd_coverage_cases.py, whose plan fields, completeness, truth and bounds tests/test_forward_coverage_cpu.py proves
without a GPU.

Every launch goes through the C entry points, into outputs that are the front of larger NaN-filled allocations: before the call
umnn_cc_launch_plan gives the case's name, P, ns and waves; afterwards umnn_last_kernel_name() is that name, umnn_launch_count() has
moved by one, every output element is written and finite and the NaNs behind each output are intact.

Bounds (see the case file): an output's U.rel_err against the float64 truth is at most M x E32, E32 the reference's own float32 error
on the same inputs (at least 2^-22), M = 8 (fp32, bf16x6, f16x3) or 64 (bf16x3); z, log_jac and ll get the absolute bounds derived
from those in flow_reference / ll_reference.  Each check prints FWDCOV|part|family|mode|id|quantity|err|E32|err / E32:
profiles/fwd_coverage/README.md tabulates the largest ratios."""
import copy
import ctypes

import numpy as np
import pytest
import torch

from tests import _fwd_coverage_cases as C
from tests import _util as U
from umnn_amd import _lib
from umnn_amd._common import _ptr, _stream
from umnn_amd.nets import mlp_spec
from umnn_amd.integral import _desc
from umnn_amd.quadrature import device_tables

pytestmark = pytest.mark.gpu
GUARD = 256             # elements behind every output
BF16 = torch.bfloat16


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


_DEVICE = {}


def _on_device(c, dev):
    """The case's net and inputs on the device as fp32 tensors (bf16-storage cases hold bf16 values); once per input set, never modified."""
    key = C._input_key(c)
    if key not in _DEVICE:
        i = C.inputs(c)
        net = copy.deepcopy(i.net).to(dev)
        _DEVICE[key] = dict(net=net, spec=mlp_spec(net), **{k: getattr(i, k).to(dev).contiguous() for k in ("x", "x0", "h", "scaling", "lj_in")})
    return _DEVICE[key]


def _out(like, dtype):
    """(whole allocation, the output: its first like.numel() elements) -- NaN everywhere"""
    big = torch.full((like.numel() + GUARD,), float("nan"), device=like.device, dtype=dtype)
    return big, big[:like.numel()].view(like.shape)


def _io(xb, hb):
    return ctypes.byref(_lib.IoDesc(_lib.DTYPE_BF16 if xb else _lib.DTYPE_F32, _lib.DTYPE_BF16 if hb else _lib.DTYPE_F32)) if (xb or hb) else None


def _expect_plan(c, desc, flags):
    info = _lib.LaunchPlanInfo()
    rc = _lib.lib().umnn_cc_launch_plan(ctypes.byref(desc), _lib.PLAN_FORWARD, c["B"], c["d"], c["E"], c["n"], flags, ctypes.byref(info))
    _lib.check(rc, "umnn_cc_launch_plan")
    got = (info.name.decode(), info.P, info.ns, info.waves_per_block)
    assert got == (c["name"], c["P"], c["ns"], c["waves"]), (c["id"], got)


def _launch(c, dev, flags, call, outs):
    """Plan check, one launch under the case's options, name / count / finiteness / guard checks.  outs: {name: (big, view)}."""
    lib = _lib.lib()
    t = _on_device(c, dev)
    desc, keep = _desc(t["spec"])
    w, s = device_tables(c["n"], dev)
    with _lib.options(**c["options"]), torch.cuda.device(dev):
        _expect_plan(c, desc, flags)
        before = lib.umnn_launch_count()
        _lib.check(call(lib, desc, w, s, _stream(dev)), c["id"])
        torch.cuda.synchronize()
        assert lib.umnn_launch_count() - before == 1, "one launch per call (an fp16-piece launch and its queued pass count as one)"
    assert lib.umnn_last_kernel_name().decode() == c["name"], (lib.umnn_last_kernel_name().decode(), c["name"])
    for nm, (big, view) in outs.items():
        assert bool(torch.isfinite(view.float()).all()), f"{c['id']}: {nm}: an element was not written, or is not finite"
        assert bool(torch.isnan(big[view.numel():].float()).all()), f"{c['id']}: the call wrote behind {nm}"
    return {nm: view for nm, (big, view) in outs.items()}


def _forward(c, dev, widen=False, alias=False):
    """umnn_cc_forward_io of the case -> {F, fx, fx0}.  widen: fp32 storage of the same (bf16-valued) inputs; alias: F is x's buffer."""
    t = _on_device(c, dev)
    xb, hb = c["x_bf16"] and not widen, c["h_bf16"] and not widen
    xdt, hdt = (BF16 if xb else torch.float32), (BF16 if hb else torch.float32)
    x, h = t["x"].to(xdt), t["h"].to(hdt)
    x0 = t["x0"].to(xdt) if c["x0"] else None
    outs = {"F": _out(x, xdt)}
    if alias:
        outs["F"][1].copy_(x)
        x = outs["F"][1]
    if not c["null_fx"]:
        outs["fx"], outs["fx0"] = _out(x, xdt), _out(x, xdt)
    p = lambda nm: _ptr(outs[nm][1]) if nm in outs else None
    call = lambda lib, desc, w, s, stream: lib.umnn_cc_forward_io(ctypes.byref(desc), _io(xb, hb), _ptr(x0), _ptr(x), _ptr(h), _ptr(w), _ptr(s), c["n"],
                                                                  c["B"], c["d"], c["E"], int(c["inv_f"]), p("F"), p("fx"), p("fx0"), stream)
    flags = (_lib.PLAN_MARKER_ALIASED if alias else 0) | (_lib.PLAN_X_BF16 if xb else 0) | (_lib.PLAN_H_BF16 if hb else 0)
    return _launch(c, dev, flags, call, outs)


def _report(c, what, err, e32):
    print(f"FWDCOV|{c['part']}|{c['family']}|{C.mode(c)}|{c['id']}|{what}|{err:.3e}|{e32:.3e}|{err / e32:.2f}")


def _against_truth(c, outs):
    r = C.reference(c)
    for nm, ref, E32, bound in zip(("F", "fx", "fx0"), (r.F, r.fx, r.fx0), r.E32, C.bounds(c)):
        if nm in outs:
            err = U.rel_err(outs[nm].double().cpu().numpy(), ref)
            _report(c, nm, err, E32)
            assert err <= bound, (c["id"], nm, err, bound, f"{err / E32:.1f} x E32, M = {C.M(c)}")
            assert err <= C.OUTER


def _same_bits(a, b, what):
    for nm in a:
        assert torch.equal(a[nm], b[nm]), f"{what}: {nm} differs in {int((a[nm] != b[nm]).sum())} elements"


def _stored(outs, xb):
    """what a bf16 store of fp32 results holds: round to nearest even"""
    return {nm: (v.to(BF16) if xb else v) for nm, v in outs.items()}


# ---- parts 1 to 3: umnn_cc_forward_io ----------------------------------------------------------------------------------------------
FORWARD_CASES = [c for c in C.CASES if c["part"] != 4]


@pytest.mark.parametrize("c", FORWARD_CASES, ids=[f"p{c['part']}-{c['id']}" for c in FORWARD_CASES])
def test_case(c, dev):
    """The case's launch: plan, name, one launch, every element written, guards intact (all in _launch), within M x E32 of the truth,
    and a second launch returns the same bits.
      bf16 storage: loads are exact widenings and stores round to nearest even, so the launch equals, bit for bit, the fp32-storage
        launch on the widened inputs (the one held to the truth), rounded to bf16.
      null-fx: F holds the bits of the launch that also writes f(x) and f(x0).
      alias (F is x's buffer, default mode): the bf16 build of the same variant runs, and the result equals the bf16x3 mode's
        non-aliased launch of the same P and ns bit for bit."""
    if c["alias"]:
        plain = dict(c, alias=False, options=dict(c["options"], **C.PREC["bf16x3"]))
        outs, ref = _forward(c, dev, alias=True), _forward(plain, dev)
        _same_bits(outs, ref, "aliased against the bf16x3 launch")
        _same_bits(outs, _forward(c, dev, alias=True), "second aliased launch")
        _against_truth(c, outs)
        return
    outs = _forward(c, dev, widen=True)
    _against_truth(c, outs)
    _same_bits(outs, _forward(c, dev, widen=True), "second launch")
    if c["null_fx"]:
        _same_bits(outs, {"F": _forward(dict(c, null_fx=False), dev)["F"]}, "F without f(x), f(x0)")
    if c["x_bf16"] or c["h_bf16"]:
        _same_bits(_forward(c, dev), _stored(outs, c["x_bf16"]), "bf16 storage against the widened launch, rounded")


@pytest.mark.parametrize("pair", C.PIPE_PAIRS, ids=[p[0]["id"] for p in C.PIPE_PAIRS])
def test_pipelined_loop_against_the_plain_loop(pair, dev):
    """fwd_pipe = 1 against fwd_pipe = 0 at fwd_p = 2: the same terms in the same order, bit-equal -- LIVE=13 and LIVE=0 (a 60-wide net
    and a zero-padded one), fp16 and bf16 pieces, node range whole and split."""
    _same_bits(_forward(pair[0], dev), _forward(pair[1], dev), "PIPE against plain")


# ---- part 4: the flow entries -------------------------------------------------------------------------------------------------------
def _flow(c, dev, widen=False, reverse=False, lj_in=None, x=None, save=False):
    """umnn_flow_stack_block_forward_io (save: _save_io with a buffer of exactly umnn_cc_forward_z2_floats) -> {z, lj, fx, fx0}.
    lj_in: None | "in" (out of place) | "alias" (log_jac is log_jac_in's buffer)."""
    t = _on_device(c, dev)
    xb, hb = c["x_bf16"] and not widen, c["h_bf16"] and not widen
    xdt, hdt = (BF16 if xb else torch.float32), (BF16 if hb else torch.float32)
    xx, h = (t["x"] if x is None else x).to(xdt), t["h"].to(hdt)
    outs = {nm: _out(xx, xdt) for nm in ("z", "lj", "fx", "fx0")}
    lin = None
    if lj_in == "in":
        lin = t["lj_in"].to(xdt)
    elif lj_in == "alias":
        outs["lj"][1].copy_(t["lj_in"].to(xdt))
        lin = outs["lj"][1]
    z2 = None
    if save:
        desc, keep = _desc(t["spec"])
        with _lib.options(**c["options"]):
            nfl = int(_lib.lib().umnn_cc_forward_z2_floats(ctypes.byref(desc), c["B"], c["d"], c["E"], c["n"]))
        assert nfl == -(-c["B"] * c["d"] // 16) * (c["n"] + 1) * ((c["hid"][1] + 4) // 4) * 64
        z2 = torch.full((nfl + GUARD,), float("nan"), device=dev)

    def call(lib, desc, w, s, stream):
        args = (ctypes.byref(desc), _io(xb, hb), _ptr(xx), _ptr(h), _ptr(t["scaling"]), _ptr(w), _ptr(s), c["n"], c["B"], c["d"], c["E"], int(reverse),
                _ptr(lin), *(_ptr(outs[nm][1]) for nm in ("z", "lj", "fx", "fx0")))
        if save:
            return lib.umnn_flow_stack_block_forward_save_io(*args, _ptr(z2), z2.numel() - GUARD, stream)
        return lib.umnn_flow_stack_block_forward_io(*args, stream)

    flags = (_lib.PLAN_Z2_SAVED if save else 0) | (_lib.PLAN_X_BF16 if xb else 0) | (_lib.PLAN_H_BF16 if hb else 0)
    res = _launch(c, dev, flags, call, outs)
    if save:
        assert bool(torch.isfinite(z2[:-GUARD]).all()) and bool(torch.isnan(z2[-GUARD:]).all()), "z_2: not all written, or written behind its size"
    return res


def _within(c, what, got, ref, bound, E32):
    err = np.abs(got.double().cpu().numpy() - ref)
    _report(c, what, U.rel_err(got.double().cpu().numpy(), ref), E32)
    worst = float((err / bound).max())
    assert worst <= 1.0, (c["id"], what, f"{worst:.2f} of the derived bound", float(err.max()))


@pytest.mark.parametrize("family", list(C.REPS))
def test_flow_block(family, dev):
    """umnn_flow_stack_block_forward_io on the family's kernel: z and log_jac within the bounds derived from bound(F) and bound(f_x)
    (flow_reference); f_x / f_x0 the bits of umnn_cc_forward's; reverse_z the same bits in reversed columns; log_jac_in added, in
    place or not; a second launch the same bits."""
    c = C.FLOW_CASES[family]["fp32"]
    r = C.flow_reference(c)
    base = _flow(c, dev)
    _within(c, "z", base["z"], r.z, r.bz, r.ref.E32[0])
    _within(c, "lj", base["lj"], r.lj, r.blj, r.ref.E32[1])
    fwd = _forward(c, dev)
    assert torch.equal(base["fx"], fwd["fx"]) and torch.equal(base["fx0"], fwd["fx0"])
    _same_bits(base, _flow(c, dev), "second launch")
    rev = _flow(c, dev, reverse=True)
    assert torch.equal(rev["z"], base["z"].flip(1)) and torch.equal(rev["lj"], base["lj"]) and torch.equal(rev["fx"], base["fx"])
    r_in = C.flow_reference(c, lj_in=True)
    added = _flow(c, dev, reverse=True, lj_in="in")
    _within(c, "lj+in", added["lj"], r_in.lj, r_in.blj, r.ref.E32[1])
    assert torch.equal(added["z"], rev["z"])
    _same_bits(added, _flow(c, dev, reverse=True, lj_in="alias"), "log_jac aliasing log_jac_in")


@pytest.mark.parametrize("family", list(C.REPS))
@pytest.mark.parametrize("storage", ["x-bf16", "h-bf16", "xh-bf16"])
def test_flow_block_bf16_storage(family, storage, dev):
    """The widen-and-round rule on the flow entry, with reverse_z and log_jac_in: the bf16-storage launch equals the fp32-storage
    launch on the widened inputs, rounded to bf16 (x-class outputs) -- the latter is held to the truth."""
    c = C.FLOW_CASES[family][storage]
    wide = _flow(c, dev, widen=True, reverse=True, lj_in="in")
    r = C.flow_reference(c, lj_in=True)
    _within(c, "z", wide["z"].flip(1), r.z, r.bz, r.ref.E32[0])
    _within(c, "lj+in", wide["lj"], r.lj, r.blj, r.ref.E32[1])
    _same_bits(_flow(c, dev, reverse=True, lj_in="in"), _stored(wide, c["x_bf16"]), "bf16 storage against the widened launch, rounded")


def test_flow_argument_errors_launch_nothing(dev):
    lib = _lib.lib()
    c = C.FLOW_CASES["f16-exact13"]["fp32"]
    t = _on_device(c, dev)
    desc, keep = _desc(t["spec"])
    w, s = device_tables(c["n"], dev)
    x = t["x"].clone()
    o = [torch.empty_like(x) for _ in range(4)]
    before = lib.umnn_launch_count()
    tail = (_ptr(w), _ptr(s), c["n"], c["B"], c["d"], c["E"])
    rc = lib.umnn_flow_stack_block_forward_io(ctypes.byref(desc), None, _ptr(x), _ptr(t["h"]), _ptr(t["scaling"]), *tail, 1, None, _ptr(x), _ptr(o[1]),
                                              _ptr(o[2]), _ptr(o[3]), _stream(dev))
    assert rc == _lib.EINVAL and b"alias" in lib.umnn_last_error()
    rc = lib.umnn_flow_stack_block_forward_io(ctypes.byref(desc), None, _ptr(x), _ptr(t["h"]), None, *tail, 0, None, _ptr(o[0]), _ptr(o[1]),
                                              _ptr(o[2]), _ptr(o[3]), _stream(dev))
    assert rc == _lib.EINVAL and b"scaling" in lib.umnn_last_error()
    torch.cuda.synchronize()
    assert lib.umnn_launch_count() == before and torch.equal(x, t["x"])


def _ll_block(c, dev, x, reverse, first, last, ll, cnt):
    t = _on_device(c, dev)
    outs = {"z": _out(x, torch.float32), "scratch": _out(x, torch.float32)}
    call = lambda lib, desc, w, s, stream: lib.umnn_flow_ll_block_forward(ctypes.byref(desc), _ptr(x), _ptr(t["h"]), _ptr(t["scaling"]), _ptr(w), _ptr(s),
                                                                          c["n"], c["B"], c["d"], c["E"], int(reverse), int(first), int(last),
                                                                          _ptr(outs["z"][1]), _ptr(outs["scratch"][1]), _ptr(ll), _ptr(cnt), stream)
    return _launch(c, dev, 0, call, outs)["z"]


@pytest.mark.parametrize("c", C.LL_CASES, ids=[c["id"] for c in C.LL_CASES])
def test_one_pass_log_likelihood(c, dev):
    """umnn_flow_ll_block_forward as a two-block chain (first on block 1, last on block 2) with rows that start and end inside tiles and
    inside P = 2 pairs: ll within the derived bound of the float64 truth (ll_reference), z the bits of the stack entry, three runs the
    same bits, the arrival counters zero afterwards and nothing written behind ll."""
    t = _on_device(c, dev)
    r = C.ll_reference(c)
    x1, x2 = t["x"], C.chain_x2(c).to(dev)
    z1, z2 = _flow(c, dev, reverse=True)["z"], _flow(c, dev, x=x2)["z"]
    runs = []
    for _ in range(3):
        cnt = torch.zeros(c["B"] + GUARD, dtype=torch.int32, device=dev)
        big, ll = _out(torch.empty(c["B"], device=dev), torch.float32)
        a = _ll_block(c, dev, x1, True, True, False, ll, cnt)
        b = _ll_block(c, dev, x2, False, False, True, ll, cnt)
        assert torch.equal(a, z1) and torch.equal(b, z2), "z of the ll entry against the stack entry"
        assert int(cnt.abs().sum()) == 0, "arrival counters are not zero again"
        assert bool(torch.isfinite(ll).all()) and bool(torch.isnan(big[c["B"]:]).all())
        runs.append(ll.clone())
    assert torch.equal(runs[0], runs[1]) and torch.equal(runs[0], runs[2])
    _within(c, "ll", runs[0], r.ll, r.bll, r.r1.ref.E32[1])


@pytest.mark.parametrize("c", C.Z2_CASES, ids=[c["id"] for c in C.Z2_CASES])
def test_saving_z2_changes_no_output(c, dev):
    """umnn_flow_stack_block_forward_save_io on every T1 x LIVE of the wide-first family: the buffer is umnn_cc_forward_z2_floats floats
    (asserted against tiles x nodes x K-steps x 64 in _flow), all of it written and nothing behind it; z, log_jac, f_x and f_x0 hold the
    bits of the launch that saves nothing.  (What the buffer holds is checked by the backward suite's saved-z_2 cases.)"""
    _same_bits(_flow(c, dev, reverse=True, lj_in="in", save=True), _flow(c, dev, reverse=True, lj_in="in"), "saving z_2")


@pytest.mark.parametrize("family", [f for f in C.REPS if f != "f16-wide-first"])
def test_saving_z2_is_unsupported_elsewhere(family, dev):
    lib = _lib.lib()
    c = C.FLOW_CASES[family]["fp32"]
    t = _on_device(c, dev)
    desc, keep = _desc(t["spec"])
    w, s = device_tables(c["n"], dev)
    o = [torch.empty_like(t["x"]) for _ in range(4)]
    z2 = torch.empty(1 << 20, device=dev)
    with _lib.options(**c["options"]):
        assert lib.umnn_cc_forward_z2_floats(ctypes.byref(desc), c["B"], c["d"], c["E"], c["n"]) == 0
        before = lib.umnn_launch_count()
        rc = lib.umnn_flow_stack_block_forward_save_io(ctypes.byref(desc), None, _ptr(t["x"]), _ptr(t["h"]), _ptr(t["scaling"]), _ptr(w), _ptr(s), c["n"],
                                                       c["B"], c["d"], c["E"], 0, None, *(_ptr(v) for v in o), _ptr(z2), z2.numel(), _stream(dev))
        assert rc == _lib.EUNSUPPORTED and lib.umnn_launch_count() == before
