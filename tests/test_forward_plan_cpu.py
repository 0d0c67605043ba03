"""The launch plan of the forward quadrature, the bracket search and the Newton solve (csrc/cc_fwd_plan.h), pinned without a GPU:
umnn_cc_launch_plan evaluates the plan of a call and launches nothing.  The expectations of tests/_fwd_plan_cases.py were derived by
reading the launchers as they were before the plan existed (see that file's docstring), boundaries included; the name alone would
not do, because P and ns change the summation order -- hence the bits -- and show in no name."""
import ctypes

import pytest

from tests import _fwd_plan_cases as C
from umnn_amd import _lib


def _plan(c, flags=None, **over):
    m = C.desc(c)
    info = _lib.LaunchPlanInfo()
    a = dict(kind=c["kind"], B=c["B"], d=c["d"], E=c["E"], n=c["n"])
    a.update(over)
    with _lib.options(**c["options"]):
        rc = _lib.lib().umnn_cc_launch_plan(ctypes.byref(m), a["kind"], a["B"], a["d"], a["E"], a["n"], c["flags"] if flags is None else flags,
                                            ctypes.byref(info))
    return rc, info


@pytest.mark.parametrize("c", C.CASES, ids=[c["id"] for c in C.CASES])
def test_plan(c):
    rc, info = _plan(c)
    assert rc == c["rc"] and info.name.decode() == c["name"]
    if rc:
        assert _lib.lib().umnn_last_error() != b""
        return
    assert (info.pieces, info.P, info.ns, info.waves_per_block, info.fallback) == (c["pieces"], c["P"], c["ns"], c["waves"], c["fallback"])
    assert info.blocks == c["blocks"]
    assert 0 < info.lds_bytes <= 160 * 1024
    if c["lds"] is not None:
        assert info.lds_bytes == c["lds"]


@pytest.mark.parametrize("c", [c for c in C.CASES if not c["rc"]][::7], ids=lambda c: c["id"])
def test_the_storage_flags_do_not_route(c):
    _, plain = _plan(c)
    _, stored = _plan(c, flags=c["flags"] | C.X_BF16 | C.H_BF16)
    for field, _type in _lib.LaunchPlanInfo._fields_:
        assert getattr(plain, field) == getattr(stored, field)


def test_an_error_is_the_entry_points_own_and_names_nothing():
    c = C.CASES[0]
    for kind in (C.FORWARD, C.SEARCH, C.SOLVE, C.SOLVE_BLOCK):
        for over in (dict(n=0), dict(d=0), dict(B=-1), dict(E=c["E"] + 1)):           # (widths[0] != 1 + E)
            rc, info = _plan(c, kind=kind, **over)
            assert rc == _lib.EINVAL and info.name == b""
    rc, info = _plan(c, kind=4)
    assert rc == _lib.EINVAL and info.name == b""
    info = _lib.LaunchPlanInfo()
    assert _lib.lib().umnn_cc_launch_plan(None, 0, 4, 2, 2, 20, 0, ctypes.byref(info)) == _lib.EINVAL and info.name == b""
    assert _lib.lib().umnn_cc_launch_plan(ctypes.byref(C.desc(c)), 0, 4, 2, c["E"], 20, 0, None) == _lib.EINVAL
    # an empty batch is no error and launches nothing
    rc, info = _plan(c, B=0)
    assert rc == 0 and info.name == b"" and info.blocks == 0
    # the texts the Python fallbacks key on
    lib = _lib.lib()
    for cid, text in (("wide-first-z2-fp32", b"two-piece arithmetic modes only"), ("z2-not-wide-first", b"not served by the wide-first kernels"),
                      ("images-exceed-lds", b"forward: weight images exceed 160 KiB of LDS"),
                      ("search-images-exceed-lds", b"invert: weight images exceed 160 KiB of LDS"),
                      ("solve-one-hidden-layer", b"solve: the matrix-core kernels need at least two hidden layers")):
        rc, _ = _plan(next(k for k in C.CASES if k["id"] == cid))
        assert rc == _lib.EUNSUPPORTED and text in lib.umnn_last_error()


def test_z2_floats_keeps_its_own_layer_bounds():
    """umnn_cc_forward_z2_floats: the plan's wide-first shape, and 2..4 layers after the cut (the three-stage backward's bound)"""
    lib = _lib.lib()
    for hid, served in (([100, 50, 50, 50, 50], True), ([100, 50, 50], True), ([100, 50], False), ([100] + [50] * 5, False),
                        ([50] * 4, False), ([100, 100, 50], False)):
        m = C.desc(dict(hid=hid, E=4))
        assert (lib.umnn_cc_forward_z2_floats(ctypes.byref(m), 40, 8, 4, 12) > 0) == served
