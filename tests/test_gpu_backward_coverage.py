"""The quadrature backward (umnn_cc_backward_io) on every kernel variant, launch plan and flag, at the smallest shapes at which each
runs: the cases of tests/_bwd_coverage_cases.py, whose names, completeness and inputs tests/test_backward_coverage_cpu.py proves
without a GPU.

Every case goes through the C entry point with a workspace of exactly umnn_cc_backward_workspace_bytes followed, in the same
allocation, by a 4 KiB byte pattern, into outputs pre-filled with NaN: the noted name is the case's, every output element is written
and finite, the pattern is intact.  A second call through integral.hip_backward takes the HIP path and returns the same bits.

Truth and criteria are those of tests/test_gpu_backward.py: tests/_truth64.backward_reference in float64 on the float32-rounded
weights and the storage-rounded inputs, U.rel_err for d_x and d_x0, U.scaled_err (max |delta| / max |ref|) for d_h and d_theta, bound
TOL = 1e-4 imported from there.  Outputs stored as bf16 get max(TOL, 2^-8) on the stored tensor (one rounding of an 8-bit
significand); d_theta is always fp32 and keeps TOL.  The inputs keep every hidden pre-activation at least GUARD away from a LeakyReLU
kink (see the case file), so the bound is an honest one.  Each case prints its four figures next to those of the reference's own
float32 arithmetic (backward_reference(dtype=float32)) on the same inputs: profiles/bwd_coverage/README.md tabulates them.

On top of TOL every output is held to the bound of its arithmetic class (the case file: arith_class, yardsticks, check_bounds): M = 8
times E32 for fp32-level outputs, 8 times max(E32, E3) for the two-piece bf16 products, d_theta flat and per parameter tensor; the
ratios are printed as BWDYARD lines.  bf16-storage cases run a second time on fp32 tensors holding the same values: that launch is held
to these bounds and the stored one to it, rounded to nearest even, bit for bit.

Kernel-against-kernel bounds are reused: the pipelined loop against the round-2 loop bit-equal in the Leibniz terms and the output
layer and 2e-6 elsewhere (tests/test_gpu_round3.py::test_software_pipelined_backward_agrees_with_the_round2_loop), the workgroup
pipeline against the pipelined loop 5e-6 (::test_weight_stationary_backward_agrees_with_the_pipelined_loop_and_fp32: the same terms, a
few additions in another order); stage C with one or two waves per tile, and on bf16 or fp16 pieces, is the latter kind of change."""
import ctypes
import copy

import pytest
import torch

import umnn_amd
from tests import _bwd_coverage_cases as C
from tests import _util as U
from tests.test_gpu_backward import TOL
from umnn_amd import _lib, integral as I
from umnn_amd._common import _ptr, _stream
from umnn_amd.nets import mlp_spec
from umnn_amd.quadrature import device_tables

pytestmark = pytest.mark.gpu
STORED_BF16 = 2.0 ** -8
SWP_VS_LOOP, WS_VS_SWP = 2e-6, 5e-6
GUARD_BYTES = 4096
NAMES = ("d_x0", "d_x", "d_h", "d_theta")
ALL = (1, 1, 1, 1)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


@pytest.fixture(autouse=True)
def _restore():
    old = umnn_amd.get_backward_precision()
    yield
    umnn_amd.set_backward_precision(old)


_DEVICE, _RUNS, _LAUNCHES = {}, {}, {}
BF16 = torch.bfloat16


def _on_device(c, dev):
    """The case's net and inputs on the device, in their storage types; built once per input set and never modified."""
    key = C._input_key(c)
    if key not in _DEVICE:
        i = C.inputs(c)
        xdt = torch.bfloat16 if c["x_bf16"] else torch.float32
        hdt = torch.bfloat16 if c["h_bf16"] else torch.float32
        to = lambda t, dt: None if t is None else t.to(dt).to(dev).contiguous()
        net = copy.deepcopy(i.net).to(dev)
        _DEVICE[key] = dict(net=net, spec=mlp_spec(net), x0=to(i.x0, xdt), x=to(i.x, xdt), h=to(i.h, hdt), g=to(i.g, xdt), g_fx=to(i.g_fx, xdt))
    return _DEVICE[key]


def _bname():
    return _lib.lib().umnn_last_kernel_name_of(_lib.PROF_BACKWARD).decode()


def _widened(t):
    """the same (bf16-valued) inputs held as fp32 tensors"""
    return dict(t, **{k: None if t[k] is None else t[k].float() for k in ("x0", "x", "h", "g", "g_fx")})


def _call(c, dev, need=ALL, widen=False):
    """One call of the C entry point under the case's options -> [d_x0, d_x, d_h, d_theta] (None where not asked for) and the
    umnn_launch_count() delta.  widen: fp32 storage of the same inputs and a null io descriptor."""
    lib = _lib.lib()
    t = _on_device(c, dev)
    if widen:
        t = _widened(t)
    B, d, E, n = c["B"], c["d"], c["E"], c["n"]
    nan = lambda like: torch.full_like(like, float("nan"))
    n_params = sum(l.weight.numel() + l.bias.numel() for l in t["spec"].linears)
    outs = [nan(t["x"]) if need[0] else None, nan(t["x"]) if need[1] else None, nan(t["h"]) if need[2] else None,
            torch.full((n_params,), float("nan"), device=dev) if need[3] else None]
    io = None
    if (c["x_bf16"] or c["h_bf16"]) and not widen:
        io = ctypes.byref(_lib.IoDesc(_lib.DTYPE_BF16 if c["x_bf16"] else _lib.DTYPE_F32, _lib.DTYPE_BF16 if c["h_bf16"] else _lib.DTYPE_F32))
    w, s = device_tables(n, dev)
    desc, keep = I._desc(t["spec"])
    pattern = (torch.arange(GUARD_BYTES, device=dev) * 37 + 11).to(torch.uint8)
    with _lib.options(**c["options"]), torch.cuda.device(dev):
        nbytes = int(lib.umnn_cc_backward_workspace_bytes(ctypes.byref(desc), B, d, E))
        assert nbytes > 0
        ws = torch.empty(nbytes + GUARD_BYTES, device=dev, dtype=torch.uint8)
        ws[nbytes:] = pattern
        before = lib.umnn_launch_count()
        rc = lib.umnn_cc_backward_io(ctypes.byref(desc), io, _ptr(t["x0"]), _ptr(t["x"]), _ptr(t["h"]), _ptr(t["g"]), _ptr(t["g_fx"]), _ptr(w),
                                     _ptr(s), n, B, d, E, int(c["inv_f"]), *(_ptr(o) for o in outs), ctypes.c_void_p(ws.data_ptr()), nbytes,
                                     _stream(dev))
        _lib.check(rc, "umnn_cc_backward_io")
        torch.cuda.synchronize()
        launches = lib.umnn_launch_count() - before
    assert _bname() == c["name"], (_bname(), c["name"])
    assert torch.equal(ws[nbytes:], pattern), "the call wrote behind umnn_cc_backward_workspace_bytes()"
    for nm, o in zip(NAMES, outs):
        assert o is None or bool(torch.isfinite(o).all()), f"{nm}: an element was not written, or is not finite"
    return outs, launches


def _through_python(c, dev, need=ALL):
    t = _on_device(c, dev)
    with _lib.options(**c["options"]):
        out = I.hip_backward(t["spec"], t["x0"], t["x"], t["h"], t["g"], t["g_fx"], c["n"], need=tuple(bool(k) for k in need), inv_f=c["inv_f"])
        torch.cuda.synchronize()
    assert umnn_amd.path_taken() == "hip" and _bname() == c["name"]
    return out


def _run(c, dev):
    """The all-outputs call of a case, once per test session."""
    if c["id"] not in _RUNS:
        outs, launches = _call(c, dev)
        assert launches == (c["launches"] or launches), (launches, c["launches"])
        _RUNS[c["id"]], _LAUNCHES[c["id"]] = outs, launches
    return _RUNS[c["id"]]


def _bounds(c):
    return (max(TOL, STORED_BF16) if c["x_bf16"] else TOL, max(TOL, STORED_BF16) if c["x_bf16"] else TOL,
            max(TOL, STORED_BF16) if c["h_bf16"] else TOL, TOL)


def _errors(outs, ref):
    crit = (U.rel_err, U.rel_err, U.scaled_err, U.scaled_err)
    return [None if o is None else crit[k](o.double().cpu().numpy(), ref[k].cpu().numpy()) for k, o in enumerate(outs)]


def _against_truth(c, outs, dev, tag=None):
    big = c["B"] * c["d"] >= 16384
    ref = C.truth(c, device=dev if big else "cpu")
    ref32 = C.truth(c, device=dev if big else "cpu", dtype=torch.float32)
    err, err32 = _errors(outs, ref), _errors(ref32, ref)
    fmt = lambda e: "|".join("-" if v is None else f"{v:.3e}" for v in e)
    print(f"BWDCOV|{c['part']}|{c['family']}|{tag or c['id']}|{fmt(err)}|{fmt(err32)}")
    for nm, e, b in zip(NAMES, err, _bounds(c)):
        assert e is None or e < b, (c["id"], nm, e, b)
    # on top: M x the yardstick of the output's arithmetic class.  (Outputs stored as bf16 carry the storage rounding: their case's
    # widened launch is held to these bounds, and the stored launch to that one bit for bit -- _widen_and_round.)
    if not (c["x_bf16"] or c["h_bf16"]):
        C.check_bounds(c, outs, ref, tag)
    return err


def _widen_and_round(c, stored, wide, what):
    """io_ld widens exactly and io_st rounds to nearest even once (cc_common.h): the launch on bf16 storage holds, bit for bit, the
    fp32-storage launch on the same values rounded to bf16 -- d_x0 and d_x under x storage, d_h under h storage --, and the same d_theta."""
    as_stored = (c["x_bf16"], c["x_bf16"], c["h_bf16"], False)
    for nm, a, b, r in zip(NAMES, stored, wide, as_stored):
        if a is None:
            continue
        want = b.to(BF16) if r else b
        assert a.dtype == want.dtype
        if not torch.equal(a, want):
            bad = a != want
            units = (a.view(torch.int16 if r else torch.int32).int() - want.view(torch.int16 if r else torch.int32).int()).abs().max()
            raise AssertionError(f"{c['id']}: {what}: {nm} differs in {int(bad.sum())} of {a.numel()} elements, by up to {int(units)} units")


def _scaled(a, b):
    return U.scaled_err(a.double().cpu().numpy(), b.double().cpu().numpy())


# ---- every case: parts 1 to 5 by name, against the truth ------------------------------------------------------------------------
@pytest.mark.parametrize("c", C.CASES, ids=[f"p{c['part']}-{c['family']}-{c['id']}" for c in C.CASES])
def test_case(c, dev):
    outs = _run(c, dev)
    again = _through_python(c, dev)
    for nm, a, b in zip(NAMES, outs, again):
        assert torch.equal(a, b), f"{nm}: a second call is not bit-equal"
    _against_truth(c, outs, dev)
    if c["x_bf16"] or c["h_bf16"]:
        wide, launches = _call(c, dev, widen=True)            # (asserts the same noted name)
        assert launches == _LAUNCHES[c["id"]], (launches, _LAUNCHES[c["id"]])
        big = c["B"] * c["d"] >= 16384
        C.check_bounds(c, wide, C.truth(c, device=dev if big else "cpu"), tag=c["id"] + "-widened")
        _widen_and_round(c, outs, wide, "bf16 storage against the widened launch, rounded")


# ---- part 2: the need masks ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("family", list(C.REP_CASES))
def test_absent_outputs_change_nothing_in_the_others(family, dev):
    """Each output switched off singly and each asked for alone (null pointers in umnn_cc_backward_io): the outputs still asked for hold
    the bits of the all-outputs call -- no kernel reorders a sum when an output is absent --, the name stays, nothing is written behind
    the workspace."""
    c = C.REP_CASES[family]
    full = _run(c, dev)
    for need in C.NEED_MASKS:
        outs, _ = _call(c, dev, need)
        for nm, k, a, b in zip(NAMES, need, outs, full):
            assert (a is None) == (not k)
            assert a is None or torch.equal(a, b), (family, need, nm, _scaled(a, b))
        py = _through_python(c, dev, need)
        assert all((a is None) == (b is None) and (a is None or torch.equal(a, b)) for a, b in zip(py, outs))


# ---- part 3: the node-range split ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("family,n", list(C.SPLIT_CASES), ids=[f"{f}-n{n}" for f, n in C.SPLIT_CASES])
def test_leibniz_terms_do_not_depend_on_the_split(family, n, dev):
    """d_x and d_x0 are written by the first and the last part of a tile's node range only: the same bits under every ns, forced
    (1, 2, 3, 7, 32 -- clamped to n + 1 by the route) and automatic.  d_h and d_theta sum the parts in another order: each case is held
    to the truth by test_case; here they are held to one another at the bound of a reordered sum (5e-6, see the module docstring)."""
    runs = [_run(c, dev) for c in C.SPLIT_CASES[family, n]]
    for c, r in zip(C.SPLIT_CASES[family, n][1:], runs[1:]):
        assert torch.equal(r[0], runs[0][0]) and torch.equal(r[1], runs[0][1]), c["id"]
        worst = max(_scaled(r[2], runs[0][2]), _scaled(r[3], runs[0][3]))
        print(f"{c['id']}: d_h / d_theta against ns=1 {worst:.2e}")
        assert worst < WS_VS_SWP, c["id"]
    # the automatic split of two tiles is 32 (clamped to n + 1 like the forced one): the same work items, the same bits
    auto, forced32 = runs[C.SPLIT_NS.index(None)], runs[C.SPLIT_NS.index(32)]
    assert all(torch.equal(a, b) for a, b in zip(auto, forced32))


# ---- kernel against kernel on the small cases ------------------------------------------------------------------------------------
@pytest.mark.parametrize("hid", [[50] * 4, [48, 60, 36, 50], [60] * 4, [50] * 3, [50] * 2, [40, 56, 33], [60, 60]], ids=C.tag)
def test_pipelined_loop_against_the_round2_loop(hid, dev):
    swp, loop = _run(C.BY_ID[f"swp-{C.tag(hid)}"], dev), _run(C.BY_ID[f"loop-{C.tag(hid)}"], dev)
    assert torch.equal(swp[0], loop[0]) and torch.equal(swp[1], loop[1])
    n_last = hid[-1] + 1
    assert torch.equal(swp[3][-n_last:], loop[3][-n_last:])
    assert _scaled(swp[2], loop[2]) < SWP_VS_LOOP and _scaled(swp[3], loop[3]) < SWP_VS_LOOP


@pytest.mark.parametrize("hid", [[50] * 4, [48, 60, 36, 50], [60] * 4], ids=C.tag)
def test_workgroup_pipeline_against_the_pipelined_loop(hid, dev):
    ws, swp = _run(C.BY_ID[f"ws-{C.tag(hid)}"], dev), _run(C.BY_ID[f"swp-{C.tag(hid)}"], dev)
    for nm, a, b in zip(NAMES, ws, swp):
        assert _scaled(a, b) < WS_VS_SWP, (nm, _scaled(a, b))


# ---- part 4: three-stage specifics -----------------------------------------------------------------------------------------------
_PART1 = {"FRONT": "front-", "FRONT_WS": "front-ws-", "FRONT_WS16": "front-ws16-"}


@pytest.mark.parametrize("family,w1,live,b2", [k for k in C.STAGE_C if k[1] in (70, 90)], ids=lambda v: str(v))
def test_stage_c_choices_agree(family, w1, live, b2, dev):
    """front_bwd2 = 0 (one wave per tile) and 2 (two waves per tile on bf16 pieces, also behind the fp16 middle stage) against 1, on
    an odd T1 (70: five tiles, the half-step image) and an even one (90: six), NL2 = 13 and 0, under the loop, WS and WS16 middle
    stages: the same terms in another order or split, 5e-6."""
    c = C.STAGE_C[family, w1, live, b2]
    one = _run(C.BY_ID[_PART1[family] + C.tag(c["hid"])], dev)
    for nm, a, b in zip(NAMES, _run(c, dev), one):
        assert _scaled(a, b) < WS_VS_SWP, (c["id"], nm, _scaled(a, b))


@pytest.mark.parametrize("key", [k for k in C.Z2_CASES if len(k) == 3], ids=lambda k: f"{k[0]}-NL2={k[1]}-{'g_fx' if k[2] else 'no-g_fx'}")
def test_saved_z2_against_the_recompute(key, dev):
    """hip_flow_block(save_z2=True) leaves hidden layer 2's pre-activations; hip_backward(z2_saved=...) skips stage A (all of it, or
    all but the tangent element of the g_fx term).  Every T1 x NL2: the name stays, both calls meet the truth, and they agree with
    one another at the bound of the same terms computed by another instruction stream (5e-6: the forward forms z_2 on fp16 pieces)."""
    c = C.Z2_CASES[key]
    t = _on_device(c, dev)
    z2 = I.hip_flow_block(t["spec"], t["x"], t["h"], torch.zeros(c["d"], device=dev), c["n"], save_z2=True)[4]
    assert z2 is not None, "umnn_cc_forward_z2_floats says the pair does not apply"
    need = (False, True, True, True)
    saved = I.hip_backward(t["spec"], None, t["x"], t["h"], t["g"], t["g_fx"], c["n"], need=need, z2_saved=z2)
    assert _bname() == c["name"] and umnn_amd.path_taken() == "hip"
    again = I.hip_backward(t["spec"], None, t["x"], t["h"], t["g"], t["g_fx"], c["n"], need=need, z2_saved=z2)
    recomputed = _run(c, dev)
    assert all(a is None or torch.equal(a, b) for a, b in zip(saved, again))
    _against_truth(c, list(saved), dev, tag=c["id"] + "-saved")
    for nm, a, b in zip(NAMES[1:], saved[1:], recomputed[1:]):
        assert _scaled(a, b) < WS_VS_SWP, (nm, _scaled(a, b))


def test_hip_backward_with_a_saved_z2_is_the_saved_entry(dev):
    """integral.hip_backward(z2_saved=z2) without an h_0 cotangent goes through umnn_cc_backward_block_io with h0_cot = NULL.  The
    entry it called before, umnn_cc_backward_saved_io, called here directly on the same tensors and workspace size (T1 = 5, NL2 = 13:
    the smallest saved-z_2 case): the same kernel name and d_x, d_h, d_theta bit for bit."""
    c = C.Z2_CASES[70, 13, True]
    t = _on_device(c, dev)
    B, d, E, n = c["B"], c["d"], c["E"], c["n"]
    lib = _lib.lib()
    nan = lambda like: torch.full_like(like, float("nan"))
    with _lib.options(**c["options"]), torch.cuda.device(dev):
        z2 = I.hip_flow_block(t["spec"], t["x"], t["h"], torch.zeros(d, device=dev), n, save_z2=True)[4]
        assert z2 is not None, "umnn_cc_forward_z2_floats says the pair does not apply"
        wrapped = I.hip_backward(t["spec"], None, t["x"], t["h"], t["g"], t["g_fx"], n, need=(False, True, True, True), z2_saved=z2)
        torch.cuda.synchronize()
        name = _bname()
        n_params = sum(l.weight.numel() + l.bias.numel() for l in t["spec"].linears)
        outs = [nan(t["x"]), nan(t["h"]), torch.full((n_params,), float("nan"), device=dev)]
        w, s = device_tables(n, dev)
        desc, keep = I._desc(t["spec"])
        nbytes = int(lib.umnn_cc_backward_workspace_bytes(ctypes.byref(desc), B, d, E))
        assert nbytes > 0
        ws = torch.empty(nbytes, device=dev, dtype=torch.uint8)
        rc = lib.umnn_cc_backward_saved_io(ctypes.byref(desc), None, _ptr(t["x"]), _ptr(t["h"]), _ptr(t["g"]), _ptr(t["g_fx"]), _ptr(w), _ptr(s),
                                           n, B, d, E, *(_ptr(o) for o in outs), _ptr(z2), int(z2.numel()), _ptr(ws), nbytes, _stream(dev))
        _lib.check(rc, "umnn_cc_backward_saved_io")
        torch.cuda.synchronize()
    assert name == _bname() == c["name"], (name, _bname(), c["name"])
    assert wrapped[0] is None
    for nm, a, b in zip(NAMES[1:], wrapped[1:], outs):
        assert a.dtype == b.dtype and torch.equal(a, b), nm


# ---- part 5: the d_h kernels by name ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key", list(C.DH), ids=lambda k: f"{k[0]}-E{k[1]}")
def test_d_h_kernel_by_name(key, dev):
    """With d_theta switched off the last finishing launch noted is the d_h kernel: cc_bwd_dh<mfma> from 32768 - 15 integrals with
    E <= 80, cc_bwd_dh below and for wider embeddings; d_h holds the bits of the all-outputs call (test_case holds those to the truth)."""
    c, name = C.DH[key]
    outs, _ = _call(c, dev, (0, 0, 1, 0))
    assert _lib.lib().umnn_last_kernel_name_of(_lib.PROF_FINISH).decode() == name
    assert torch.equal(outs[2], _run(c, dev)[2])


# ---- part 4: the saved-z2 pair with a bf16 embedding, at the C entries -------------------------------------------------------------
def _saved_pair(c, dev, widen, h0=None):
    """umnn_flow_stack_block_forward_save_io into a z_2 buffer of exactly umnn_cc_forward_z2_floats floats, then
    umnn_cc_backward_saved_io on it (h0 given: umnn_cc_backward_block_io, which adds h0 [B, d] into embedding row 0 of d_h before the
    store), both with the case's io descriptor (widen: the same values as fp32 tensors, io = NULL).  Outputs
    pre-filled with NaN, the workspace exactly sized and followed by the byte pattern, NaN behind z_2 -> ([None, d_x, d_h, d_theta],
    z_2, the backward's launch count)."""
    lib = _lib.lib()
    t = _widened(_on_device(c, dev)) if widen else _on_device(c, dev)
    B, d, E, n = c["B"], c["d"], c["E"], c["n"]
    hb = c["h_bf16"] and not widen
    io = ctypes.byref(_lib.IoDesc(_lib.DTYPE_F32, _lib.DTYPE_BF16)) if hb else None
    assert t["x"].dtype == torch.float32 and t["h"].dtype == (BF16 if hb else torch.float32) and t["x0"] is None
    nan = lambda like: torch.full_like(like, float("nan"))
    n_params = sum(l.weight.numel() + l.bias.numel() for l in t["spec"].linears)
    w, s = device_tables(n, dev)
    desc, keep = I._desc(t["spec"])
    scaling = torch.zeros(d, device=dev)
    fwd = [nan(t["x"]) for _ in range(4)]
    outs = [None, nan(t["x"]), nan(t["h"]), torch.full((n_params,), float("nan"), device=dev)]
    pattern = (torch.arange(GUARD_BYTES, device=dev) * 37 + 11).to(torch.uint8)
    with _lib.options(**c["options"]), torch.cuda.device(dev):
        nfl = int(lib.umnn_cc_forward_z2_floats(ctypes.byref(desc), B, d, E, n))
        assert nfl == -(-B * d // 16) * (n + 1) * ((c["hid"][1] + 4) // 4) * 64
        z2 = torch.full((nfl + GUARD_BYTES,), float("nan"), device=dev)
        rc = lib.umnn_flow_stack_block_forward_save_io(ctypes.byref(desc), io, _ptr(t["x"]), _ptr(t["h"]), _ptr(scaling), _ptr(w), _ptr(s), n, B, d,
                                                       E, 0, None, *(_ptr(o) for o in fwd), _ptr(z2), nfl, _stream(dev))
        _lib.check(rc, "umnn_flow_stack_block_forward_save_io")
        torch.cuda.synchronize()
        assert bool(torch.isfinite(z2[:nfl]).all()) and bool(torch.isnan(z2[nfl:]).all()), "z_2: not all written, or written behind its size"
        assert all(bool(torch.isfinite(o).all()) for o in fwd)
        nbytes = int(lib.umnn_cc_backward_workspace_bytes(ctypes.byref(desc), B, d, E))
        assert nbytes > 0
        ws = torch.empty(nbytes + GUARD_BYTES, device=dev, dtype=torch.uint8)
        ws[nbytes:] = pattern
        before = lib.umnn_launch_count()
        head = (ctypes.byref(desc), io, _ptr(t["x"]), _ptr(t["h"]), _ptr(t["g"]), _ptr(t["g_fx"]), _ptr(w), _ptr(s), n, B, d, E)
        tail = (*(_ptr(o) for o in outs[1:]), _ptr(z2), nfl, ctypes.c_void_p(ws.data_ptr()), nbytes, _stream(dev))
        rc = lib.umnn_cc_backward_saved_io(*head, *tail) if h0 is None else lib.umnn_cc_backward_block_io(*head, _ptr(h0), *tail)
        _lib.check(rc, "umnn_cc_backward_saved_io / _block_io")
        torch.cuda.synchronize()
        launches = lib.umnn_launch_count() - before
    assert _bname() == c["name"], (_bname(), c["name"])
    assert torch.equal(ws[nbytes:], pattern), "the call wrote behind umnn_cc_backward_workspace_bytes()"
    assert bool(torch.isnan(z2[nfl:]).all())
    for nm, o in zip(NAMES[1:], outs[1:]):
        assert bool(torch.isfinite(o).all()), f"{nm}: an element was not written, or is not finite"
    return outs, z2[:nfl], launches


@pytest.mark.parametrize("key", [k for k in C.Z2_CASES if len(k) == 4], ids=lambda k: f"{k[0]}-NL2={k[1]}-g_fx-{k[3]}")
def test_saved_z2_pair_with_a_bf16_embedding(key, dev):
    """The MNIST-shaped training path at the C entries, T1 = 5 and 8, NL2 = 13 and 0: the three-stage name; the pair on fp32 storage of
    the same values within the class B bounds of the truth; the pair on bf16 storage leaves the same z_2 and holds that pair's d_h
    rounded to bf16, its d_x and d_theta, bit for bit; saved against recomputed (umnn_cc_backward_io, fp32 storage of the same values:
    two stored d_h may differ by a whole bf16 unit) within 5e-6."""
    c = C.Z2_CASES[key]
    stored, z2_stored, launches = _saved_pair(c, dev, widen=False)
    wide, z2_wide, launches_wide = _saved_pair(c, dev, widen=True)
    assert launches == launches_wide and torch.equal(z2_stored, z2_wide)
    assert stored[2].dtype == BF16 and wide[2].dtype == torch.float32
    ref = C.truth(c)
    err = _errors(wide, ref)
    print(f"BWDCOV|{c['part']}|{c['family']}|{c['id']}-saved-widened|" + "|".join("-" if v is None else f"{v:.3e}" for v in err))
    for nm, e in zip(NAMES, err):
        assert e is None or e < TOL, (c["id"], nm, e)
    C.check_bounds(c, wide, ref, tag=c["id"] + "-saved-widened")
    _widen_and_round(c, stored, wide, "the saved pair on bf16 storage against the widened pair, rounded")
    for nm, e, b in zip(NAMES, _errors(stored, ref), _bounds(c)):
        assert e is None or e < b, (c["id"], nm, e, b)
    recomputed, _ = _call(c, dev, widen=True)
    for nm, a, b in zip(NAMES[1:], wide[1:], recomputed[1:]):
        assert _scaled(a, b) < WS_VS_SWP, (nm, _scaled(a, b))
    for nm, a, b in ((NAMES[1], stored[1], _run(c, dev)[1]), (NAMES[3], stored[3], _run(c, dev)[3])):
        assert _scaled(a, b) < WS_VS_SWP, (nm, _scaled(a, b))
    # the block entry: the h_0 cotangent goes into embedding row 0 of d_h in fp32, before the one store
    h0 = _on_device(c, dev)["g"]
    wide_h0, _, n_wide = _saved_pair(c, dev, widen=True, h0=h0)
    stored_h0, _, n_stored = _saved_pair(c, dev, widen=False, h0=h0)
    assert n_wide == n_stored == launches
    _plus_h0(c, wide, wide_h0, h0)
    _widen_and_round(c, stored_h0, wide_h0, "the block entry on bf16 storage against the widened one, rounded")


def _plus_h0(c, plain, with_h0, h0):
    """d_h with the h_0 term is d_h without it plus h0 in embedding row 0 (one fp32 addition: the same bits), every other output the same"""
    want = plain[2].clone()
    want.view(c["B"], c["E"], c["d"])[:, 0, :] += h0
    assert torch.equal(with_h0[2], want), "d_h"
    assert all(a is None and b is None or torch.equal(a, b) for k, (a, b) in enumerate(zip(plain, with_h0)) if k != 2)


def _block_call(c, dev, h0, need=ALL):
    """umnn_cc_backward_block_io without a saved z_2 (lower limit 0; the case's x0 is not used), exactly-sized workspace and guard."""
    lib = _lib.lib()
    t = _on_device(c, dev)
    assert not (c["x_bf16"] or c["h_bf16"])
    B, d, E, n = c["B"], c["d"], c["E"], c["n"]
    nan = lambda like: torch.full_like(like, float("nan"))
    n_params = sum(l.weight.numel() + l.bias.numel() for l in t["spec"].linears)
    outs = [None, nan(t["x"]) if need[1] else None, nan(t["h"]) if need[2] else None, torch.full((n_params,), float("nan"), device=dev) if need[3] else None]
    w, s = device_tables(n, dev)
    desc, keep = I._desc(t["spec"])
    pattern = (torch.arange(GUARD_BYTES, device=dev) * 37 + 11).to(torch.uint8)
    with _lib.options(**c["options"]), torch.cuda.device(dev):
        nbytes = int(lib.umnn_cc_backward_workspace_bytes(ctypes.byref(desc), B, d, E))
        ws = torch.empty(nbytes + GUARD_BYTES, device=dev, dtype=torch.uint8)
        ws[nbytes:] = pattern
        rc = lib.umnn_cc_backward_block_io(ctypes.byref(desc), None, _ptr(t["x"]), _ptr(t["h"]), _ptr(t["g"]), _ptr(t["g_fx"]), _ptr(w), _ptr(s), n, B, d,
                                           E, _ptr(h0), *(_ptr(o) for o in outs[1:]), None, 0, ctypes.c_void_p(ws.data_ptr()), nbytes, _stream(dev))
        _lib.check(rc, "umnn_cc_backward_block_io")
        torch.cuda.synchronize()
    assert torch.equal(ws[nbytes:], pattern), "the call wrote behind umnn_cc_backward_workspace_bytes()"
    assert all(o is None or bool(torch.isfinite(o).all()) for o in outs)
    return outs


# ---- the fused training block on a bf16 embedding: d_h is rounded once, row 0 included ----------------------------------------------
@pytest.mark.parametrize("reverse_z", [False, True], ids=["forward-z", "reverse-z"])
def test_flow_block_vjp_rounds_d_h_once(reverse_z, dev):
    """FlowBlockTransform (B = 41, d = 3, E = 4, 50-50-50-50, n = 6; every g_z and g_log_jac non-zero) with the embedding h in bf16, and
    with the same values in fp32: z carries h_0 = embedding row 0, so d_h row 0 is the quadrature's plus the cotangent of F.  The bf16
    run's d_h is the fp32 run's rounded to bf16 once, bit for bit, in every row; d_x and the parameter gradients are the same bits."""
    c = C.BY_ID["rep-SWP-h-bf16"]
    assert (c["B"], c["d"], c["E"], c["hid"], c["n"]) == (41, 3, 4, [50] * 4, 6)
    t = _on_device(c, dev)
    B, d, E = c["B"], c["d"], c["E"]
    scaling = torch.linspace(-0.3, 0.3, d, device=dev)
    gz, glj = t["g"], t["g_fx"]
    assert bool((gz != 0).all()) and bool((glj != 0).all())
    params = list(t["net"].parameters())

    def run(h):
        x, h = t["x"].clone().requires_grad_(), h.clone().requires_grad_()
        z, lj = I.FlowBlockTransform.apply(x, t["net"], h, scaling, c["n"], reverse_z, None, *params)
        grads = torch.autograd.grad((z, lj), (x, h, *params), (gz, glj))
        assert umnn_amd.path_taken() == "hip"
        return grads, _bname()

    (dx16, dh16, *dth16), name16 = run(t["h"])
    (dx32, dh32, *dth32), name32 = run(t["h"].float())
    assert name16 == name32 and dh16.dtype == BF16 and dh32.dtype == torch.float32
    assert torch.equal(dx16, dx32), "d_x"
    assert all(torch.equal(a, b) for a, b in zip(dth16, dth32)), "parameter gradients"
    bad = (dh16 != dh32.to(BF16)).view(B, E, d)
    rows = [int(bad[:, e, :].sum()) for e in range(E)]
    print(f"d_h elements that are not the fp32 run's rounded once, per embedding row: {rows} of {B * d} each")
    assert rows == [0] * E, rows


@pytest.mark.parametrize("key", list(C.DH), ids=lambda k: f"{k[0]}-E{k[1]}")
def test_d_h_kernels_add_the_h0_cotangent_before_the_store(key, dev):
    """umnn_cc_backward_block_io on both d_h kernels (by name), every E of part 5 (one, a tile less one, a tile, a tile and one, five
    tiles, above the matrix-core kernel's limit), integral counts that end a tile early, exactly and one in: with h0 the call returns the
    d_h of the call without it plus h0 in embedding row 0 and nowhere else -- the same bits as the fp32 addition --, and the same d_x and
    d_theta; d_h alone holds the bits of the all-outputs call."""
    c, name = C.DH[key]
    h0 = _on_device(c, dev)["g"]
    plain, with_h0 = _block_call(c, dev, None), _block_call(c, dev, h0)
    _plus_h0(c, plain, with_h0, h0)
    alone = _block_call(c, dev, h0, (0, 0, 1, 0))
    assert _lib.lib().umnn_last_kernel_name_of(_lib.PROF_FINISH).decode() == name
    assert torch.equal(alone[2], with_h0[2])
