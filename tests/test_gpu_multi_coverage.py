"""The multi-output quadrature kernels (csrc/cc_multi.hip) on every family, backward pass, plan and flag, at the smallest shapes at
which each runs: the cases of tests/_multi_coverage_cases.py, whose names, completeness and inputs tests/test_multi_coverage_cpu.py
proves without a GPU.

Every call goes through umnn_cc_forward_multi / umnn_cc_backward_multi themselves (ctypes), into outputs pre-filled with NaN with
GUARD_FLOATS more NaNs behind each in the same allocation, and -- the backward -- with a workspace of exactly
umnn_cc_backward_multi_workspace_bytes filled with 0xFF bytes (NaNs to whoever reads a slice no launch wrote) and a byte pattern
behind it: the noted names and the launch-count delta are the case's, every output element is written and finite, the guards are
intact.  Two backward calls return the same bits.

Truth and bounds: `truth` / `bound` of the case file -- the float64 quadrature on the float32-rounded weights, inputs and tables, each
output within M x E32 of it (E32: the float32 run of the same function, floor 2^-22; never above 1e-5).  Each case prints its
figures as multiples of E32: profiles/multi_coverage/README.md tabulates them."""
import ctypes
import types

import numpy as np
import pytest
import torch

from tests import _multi_coverage_cases as C
from umnn_amd import _lib
from umnn_amd._common import _ptr, _stream
from umnn_amd.quadrature import device_tables

pytestmark = pytest.mark.gpu
GUARD_FLOATS, GUARD_BYTES = 1024, 4096
NAN_BITS = 0x7FC00000
ALL = (1, 1, 1, 1)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


_DEVICE = {}


def _on_device(c, dev, guard=C.GUARD):
    """The case's weights and inputs on the device in float32, and its struct umnn_mlp; built once per input set, never modified."""
    key = C._input_key(c) + (guard,)
    if key not in _DEVICE:
        i = C.inputs(c, guard)
        to = lambda t: None if t is None else t.float().to(dev).contiguous()
        lins = [m for m in i.net.net if isinstance(m, torch.nn.Linear)]
        W, b = [to(l.weight.detach()) for l in lins], [to(l.bias.detach()) for l in lins]
        m = C.desc(c)
        for l in range(len(lins)):
            m.W[l], m.b[l] = W[l].data_ptr(), b[l].data_ptr()
        _DEVICE[key] = types.SimpleNamespace(desc=m, W=W, b=b, x0=to(i.x0), x=to(i.x), h=to(i.h), g=to(i.g), shapes=[p.shape for p in i.net.net.parameters()],
                                             dummy=torch.zeros(16, device=dev))
    return _DEVICE[key]


class _Out:
    """A float32 output of `numel` elements pre-filled with NaN, with GUARD_FLOATS NaNs behind it"""

    def __init__(self, shape, dev):
        self.n = int(np.prod(shape))
        self.buf = torch.full((self.n + GUARD_FLOATS,), float("nan"), device=dev)
        self.t = self.buf[:self.n].view(*shape)

    def check(self, name):
        assert bool((self.buf[self.n:].view(torch.int32) == NAN_BITS).all()), f"{name}: written behind its last element"
        assert bool(torch.isfinite(self.t).all()), f"{name}: an element was not written, or is not finite"
        return self.t


def _rows(t, lo, hi):
    sl = lambda v: None if v is None else v[lo:hi]
    return sl(t.x0), sl(t.x), sl(t.h), sl(t.g)


def _hptr(t, h):
    return _ptr(h) if h.numel() else _ptr(t.dummy)          # (E = 0: the entries still want a pointer)


def _forward(c, t, dev, lo=0, hi=None, fx=True):
    """-> (F, f_x, f_x0 [B, d, K] or None, name, launches) of sample rows lo..hi"""
    lib = _lib.lib()
    x0, x, h, _ = _rows(t, lo, c["B"] if hi is None else hi)
    B, d, K = x.shape[0], c["d"], c["K"]
    outs = [_Out((B, d, K), dev), _Out((B, d, K), dev) if fx else None, _Out((B, d, K), dev) if fx else None]
    w, s = device_tables(c["n"], dev)
    with torch.cuda.device(dev):
        before = lib.umnn_launch_count()
        rc = lib.umnn_cc_forward_multi(ctypes.byref(t.desc), _ptr(x0), _ptr(x), _hptr(t, h), _ptr(w), _ptr(s), c["n"], B, d, c["E"], int(c["inv_f"]),
                                       *(None if o is None else _ptr(o.t) for o in outs), _stream(dev))
        _lib.check(rc, "umnn_cc_forward_multi")
        torch.cuda.synchronize()
        launches = lib.umnn_launch_count() - before
    name = lib.umnn_last_kernel_name().decode()
    return [None if o is None else o.check(nm) for nm, o in zip(C.VALUES, outs)] + [name, launches]


def _backward(c, t, dev, need=ALL, lo=0, hi=None):
    """-> ([d_x0, d_x, d_h, d_theta], None where not asked for; name of the last pass; launches) of sample rows lo..hi"""
    lib = _lib.lib()
    x0, x, h, g = _rows(t, lo, c["B"] if hi is None else hi)
    B, d, E = x.shape[0], c["d"], c["E"]
    shapes = [(B, d), (B, d), (B, E * d), (C.n_params(c),)]
    outs = [_Out(sh, dev) if k and int(np.prod(sh)) else None for k, sh in zip(need, shapes)]
    w, s = device_tables(c["n"], dev)
    pattern = (torch.arange(GUARD_BYTES, device=dev) * 37 + 11).to(torch.uint8)
    with torch.cuda.device(dev):
        nbytes = int(lib.umnn_cc_backward_multi_workspace_bytes(ctypes.byref(t.desc), B, d, E))
        assert nbytes > 0, lib.umnn_last_error()
        ws = torch.empty(nbytes + GUARD_BYTES, device=dev, dtype=torch.uint8)
        ws[:nbytes] = 0xFF
        ws[nbytes:] = pattern
        before = lib.umnn_launch_count()
        rc = lib.umnn_cc_backward_multi(ctypes.byref(t.desc), _ptr(x0), _ptr(x), _hptr(t, h), _ptr(g), _ptr(w), _ptr(s), c["n"], B, d, E, int(c["inv_f"]),
                                        *(None if o is None else _ptr(o.t) for o in outs), ctypes.c_void_p(ws.data_ptr()), nbytes, _stream(dev))
        _lib.check(rc, "umnn_cc_backward_multi")
        torch.cuda.synchronize()
        launches = lib.umnn_launch_count() - before
    assert torch.equal(ws[nbytes:], pattern), "the call wrote behind umnn_cc_backward_multi_workspace_bytes()"
    name = lib.umnn_last_kernel_name_of(_lib.PROF_BACKWARD).decode()
    return [None if o is None else o.check(nm) for nm, o in zip(C.GRADS, outs)], name, launches


def _as_rows(c, t, fwd, bwd):
    """kernel outputs in the layout of the truth: the B d row problem, d_theta one array per parameter tensor"""
    B, d, E, K = fwd[0].shape[0] if fwd else bwd[1].shape[0], c["d"], c["E"], c["K"]
    np_ = lambda v: None if v is None else v.double().cpu().numpy()
    got = types.SimpleNamespace()
    if fwd:
        got.F, got.fx, got.fx0 = (None if v is None else np_(v).reshape(B * d, K) for v in fwd[:3])
    if bwd:
        got.dx0, got.dx = (None if v is None else np_(v).reshape(B * d) for v in bwd[:2])
        got.dh = None if bwd[2] is None else np_(bwd[2].view(B, E, d).transpose(1, 2).reshape(B * d, E))
        got.dtheta = None
        if bwd[3] is not None:
            flat, got.dtheta, o = np_(bwd[3]), [], 0
            for sh in t.shapes:
                got.dtheta.append(flat[o:o + int(np.prod(sh))].reshape(*sh))
                o += int(np.prod(sh))
            assert o == flat.size
    return got


def _against_truth(c, got, T, tag=None):
    err, worst = C.errors(got, T.t), {}
    for name, e in err.items():
        es, Es = (e, T.E32[name]) if isinstance(e, list) else ([e], [T.E32[name]])
        worst[name] = max(a / b for a, b in zip(es, Es))
    print(f"MULTICOV|{c['part']}|{c['fam'][0]},{c['fam'][1]}|{tag or c['id']}|" + "|".join(f"{k} {v:.2f}" for k, v in worst.items())
          + "|E32 " + " ".join(f"{k} {(max(v) if isinstance(v, list) else v):.2e}" for k, v in T.E32.items() if k in err))
    for name, e in err.items():
        es, Es = (e, T.E32[name]) if isinstance(e, list) else ([e], [T.E32[name]])
        for j, (a, b) in enumerate(zip(es, Es)):
            assert a <= C.bound(b, name), (c["id"], name, j, a, C.bound(b, name))
    return worst


def _equal(a, b):
    return (a is None and b is None) or torch.equal(a, b)


_FULL = {}


def _full(c, dev):
    """forward and all-outputs backward of a case, checked by name and count; once per session"""
    if c["id"] not in _FULL:
        t = _on_device(c, dev)
        *fwd, fname, fl = _forward(c, t, dev)
        assert fname == c["fwd"] and fl == 1, (fname, fl)
        bwd, bname, bl = _backward(c, t, dev)
        assert bname == c["last"] and bl == c["passes"], (bname, bl)
        _FULL[c["id"]] = (fwd, bwd)
    return _FULL[c["id"]]


# ---- parts 1 to 3: every case by name, against the truth -------------------------------------------------------------------------
@pytest.mark.parametrize("c", C.CASES, ids=[f"{c['fam'][0]}x{c['fam'][1]}-{c['id']}" for c in C.CASES])
def test_case(c, dev):
    t = _on_device(c, dev)
    fwd, bwd = _full(c, dev)
    again, _, _ = _backward(c, t, dev)
    for nm, a, b in zip(C.GRADS, bwd, again):
        assert _equal(a, b), f"{nm}: a second call is not bit-equal"
    # without d_theta: the first pass alone, by name; what it writes holds the bits of the full call
    alone, name, launches = _backward(c, t, dev, (1, 1, 1, 0))
    assert name == c["first"] and launches == 1, (name, launches)
    for nm, a, b in zip(C.GRADS[:3], bwd, alone):
        assert _equal(a, b), f"{nm}: differs when d_theta is not asked for"
    _against_truth(c, _as_rows(c, t, fwd, bwd), C.truth(c))


# ---- part 2: absent outputs ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fam", list(C.REP_CASES), ids=lambda f: f"{f[0]}x{f[1]}")
def test_absent_outputs_change_nothing_in_the_others(fam, dev):
    """Every subset of (d_x0, d_x, d_h, d_theta) as null pointers: the outputs still asked for hold the bits of the all-outputs call;
    the passes run are the case's with d_theta and the first alone without; nothing is written behind an output or the workspace.
    The forward with f_x and f_x0 null: the same F."""
    c = C.REP_CASES[fam]
    t = _on_device(c, dev)
    fwd, bwd = _full(c, dev)
    for need in C.NEED_MASKS:
        outs, name, launches = _backward(c, t, dev, need)
        assert (name, launches) == ((c["last"], c["passes"]) if need[3] else (c["first"], 1)), (need, name, launches)
        for nm, k, a, b in zip(C.GRADS, need, outs, bwd):
            assert (a is None) == (not k) and (a is None or torch.equal(a, b)), (fam, need, nm)
    F, fx, fx0, name, _ = _forward(c, t, dev, fx=False)
    assert fx is None and fx0 is None and name == c["fwd"] and torch.equal(F, fwd[0])


# ---- part 4: large launches ---------------------------------------------------------------------------------------------------------
def _chunks(c, cus):
    """sample-row ranges of at most CHUNK_INTEGRALS integrals, below every threshold of the two entries on this device"""
    rows = C.CHUNK_INTEGRALS // c["d"]
    tiles = (rows * c["d"] + 15) // 16
    assert tiles < 2 * 4 * cus and tiles <= 4 * cus and rows * c["d"] // 64 < 2 * cus and rows * c["d"] <= 65536
    return [(lo, min(lo + rows, c["B"])) for lo in range(0, c["B"], rows)]


@pytest.mark.parametrize("which", [0, 1], ids=["A", "B"])
def test_large_launch_equals_its_chunks(which, dev):
    """Shape A (2 x 4 x CUs + 3 tiles, d = 1): two point tiles per forward wave with a dead last one, persistent backward waves of two
    and three groups, the 64-integral d_h workgroups, ceil(NI / 64) first-layer parts.  Shape B (65538 integrals, d = 3): 1024 parts of
    65.  Every per-row output holds the bits of launches of the same rows in chunks below every threshold (P = 1, one group per
    wave, 16-integral d_h workgroups, parts of 64); d_theta -- and the rest -- meet the float64 truth."""
    cus = torch.cuda.get_device_properties(dev).multi_processor_count
    c = C.large_case(C.large_shapes(cus)[which])
    NI, tiles = c["B"] * c["d"], (c["B"] * c["d"] + 15) // 16
    assert tiles >= 2 * 4 * cus and tiles % 2 == 1 and tiles > 2 * 4 * cus and NI // 64 >= 2 * cus
    assert which == 0 or -(-NI // 1024) == 65
    t = _on_device(c, dev)
    *fwd, fname, _ = _forward(c, t, dev)
    assert fname == c["fwd"] == C.fwd_name(2, 8, 2)
    bwd, bname, launches = _backward(c, t, dev)
    assert bname == c["last"] and launches == c["passes"]
    again, _, _ = _backward(c, t, dev)
    assert all(_equal(a, b) for a, b in zip(bwd, again))
    for lo, hi in _chunks(c, cus):
        *f1, name1, _ = _forward(c, t, dev, lo, hi)
        assert name1 == C.fwd_name(2, 8, 1)
        for nm, a, b in zip(C.VALUES, f1, fwd):
            assert torch.equal(a, b[lo:hi]), (nm, lo)
        b1, _, _ = _backward(c, t, dev, (1, 1, 1, 0), lo, hi)
        for nm, a, b in zip(C.GRADS[:3], b1, bwd):
            assert torch.equal(a, b[lo:hi]), (nm, lo)
    _against_truth(c, _as_rows(c, t, fwd, bwd), C.truth(c))


@pytest.mark.parametrize("fam", [f for f in C.REPS if f != (2, 8)], ids=lambda f: f"{f[0]}x{f[1]}")
def test_large_forward_equals_its_chunks(fam, dev):
    """The P = 2 instantiation of the other four families at shape A: by name, bit-equal to P = 1 launches of the same rows, and
    against the float64 truth on the first and the last 32 rows (the dead second tile sits behind the last)."""
    cus = torch.cuda.get_device_properties(dev).multi_processor_count
    c = C.large_case(C.large_shapes(cus)[0], fam, C.REPS[fam][0])
    t = _on_device(c, dev, guard=0)
    *fwd, fname, _ = _forward(c, t, dev)
    assert fname == C.fwd_name(*fam, 2)
    for lo, hi in _chunks(c, cus):
        *f1, name1, _ = _forward(c, t, dev, lo, hi)
        assert name1 == C.fwd_name(*fam, 1)
        for nm, a, b in zip(C.VALUES, f1, fwd):
            assert torch.equal(a, b[lo:hi]), (nm, lo)
    rows = np.r_[0:32, c["B"] - 32:c["B"]]
    T = C.truth(c, guard=0, rows=rows, grads=False)
    got = types.SimpleNamespace(**{nm: v.double().cpu().numpy().reshape(c["B"], c["K"])[rows] for nm, v in zip(C.VALUES, fwd)})
    _against_truth(c, got, T)


# ---- part 5: the empty batch ------------------------------------------------------------------------------------------------------
def test_empty_batch_at_the_c_entry(dev):
    c = C.BY_ID["p1-20x31x9"]
    t = _on_device(c, dev)
    lib = _lib.lib()
    w, s = device_tables(c["n"], dev)
    p = _ptr(t.dummy)
    dth = torch.full((C.n_params(c) + GUARD_FLOATS,), float("nan"), device=dev)
    with torch.cuda.device(dev):
        before = lib.umnn_launch_count()
        assert lib.umnn_cc_forward_multi(ctypes.byref(t.desc), None, p, p, _ptr(w), _ptr(s), c["n"], 0, c["d"], c["E"], 0, p, p, p, _stream(dev)) == 0
        assert lib.umnn_cc_backward_multi(ctypes.byref(t.desc), None, p, p, p, _ptr(w), _ptr(s), c["n"], 0, c["d"], c["E"], 0, p, p, p, _ptr(dth),
                                          None, 0, _stream(dev)) == 0
        torch.cuda.synchronize()
        assert lib.umnn_launch_count() == before
    assert bool((dth[:C.n_params(c)] == 0).all()) and bool((dth[C.n_params(c):].view(torch.int32) == NAN_BITS).all())
    assert bool((t.dummy == 0).all())
