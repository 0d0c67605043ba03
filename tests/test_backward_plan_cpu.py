"""The launch plan of the quadrature backward (csrc/cc_bwd_plan.h), pinned without a GPU: umnn_cc_backward_plan_name evaluates the
shape plan and the route of a call and launches nothing.  The expected names of tests/_bwd_plan_cases.py were derived by reading the
launchers as they were before the plan header existed (see that file's docstring), boundaries included."""
import ctypes

import pytest

from tests import _bwd_plan_cases as C
from umnn_amd import _lib


def _plan_name(c, B=None):
    m = C.desc(c)
    with _lib.options(**c["options"]):
        return _lib.lib().umnn_cc_backward_plan_name(ctypes.byref(m), c["B"] if B is None else B, c["d"], c["E"], c["n"], c["flags"]).decode()


def _workspace(c, B):
    m = C.desc(c)
    with _lib.options(**c["options"]):
        return _lib.lib().umnn_cc_backward_workspace_bytes(ctypes.byref(m), B, c["d"], c["E"])


@pytest.mark.parametrize("c", C.CASES, ids=[c["id"] for c in C.CASES])
def test_plan_name(c):
    assert _plan_name(c) == c["name"]


@pytest.mark.parametrize("c", C.CASES, ids=[c["id"] for c in C.CASES])
def test_workspace_is_monotonic_and_fails_where_the_plan_does(c):
    """The size umnn_cc_backward_workspace_bytes reports is the shape plan's: never smaller for one more sample, and -1 exactly
    where the plan has no kernel for the shape.  (B d = 1024 x 16 is where the dW1 finishing kernel's chunk doubles, so B = 1023
    has 1023 partial slices where B = 1024 has 512: the plan sizes that region, and the node-split ones, by bounds that only grow.)"""
    ws, ws_less = _workspace(c, c["B"]), _workspace(c, c["B"] - 1)
    assert (ws == -1) == (c["name"] == "")
    if c["name"]:
        assert ws > 0 and ws >= ws_less >= 0
    else:
        assert ws_less == -1


@pytest.mark.parametrize("options", [{}, {"bwd_ns": 4}], ids=["default", "bwd_ns=4"])
@pytest.mark.parametrize("hid,E,d", [([50] * 4, 30, 16), ([50] * 4, 30, 3), ([100, 50, 50, 50, 50], 4, 63), ([20, 20], 4, 1)])
def test_workspace_never_shrinks_with_the_batch(hid, E, d, options):
    """Every B up to past the last place where a count of the plan jumps at 256 CUs (the node-range split ends above B d = 8192,
    the dW1 chunk last doubles at B d = 32768)."""
    m = C.desc(dict(hid=hid, E=E, out_act=C.ELU))
    with _lib.options(**options):
        sizes = [_lib.lib().umnn_cc_backward_workspace_bytes(ctypes.byref(m), B, d, E) for B in range(1, 33000 // d + 2)]
    assert sizes[0] > 0 and all(b >= a for a, b in zip(sizes, sizes[1:]))


def test_plan_name_is_empty_where_the_call_returns_an_error():
    c = C.CASES[0]
    m = C.desc(c)
    name = _lib.lib().umnn_cc_backward_plan_name
    assert name(ctypes.byref(m), c["B"], c["d"], c["E"], 0, 0) == b""            # nb_steps < 1
    assert name(ctypes.byref(m), c["B"], 0, c["E"], c["n"], 0) == b""            # d < 1
    assert name(ctypes.byref(m), c["B"], c["d"], c["E"] + 1, c["n"], 0) == b""   # widths[0] != 1 + E
    assert name(None, c["B"], c["d"], c["E"], c["n"], 0) == b""
    # the storage flags do not route
    assert name(ctypes.byref(m), c["B"], c["d"], c["E"], c["n"], _lib.PLAN_X_BF16 | _lib.PLAN_H_BF16) == c["name"].encode()


@pytest.mark.parametrize("hid,E,kind", [
    ([100, 50, 50], 4, 1), ([72, 72], 4, 1), ([120, 40, 40, 40], 4, 1), ([100, 50, 50, 50, 50], 4, 1),       # three-stage / zero-padded
    ([64, 64], 5, 1), ([64, 64, 64, 64], 5, 1), ([100, 100, 100], 5, 1),                                     # shape-exact families
    ([50] * 4, 30, 1), ([48, 60, 36, 50], 30, 0), ([20, 20], 4, 0),
    ([100, 80, 70, 90, 70], 4, -1), ([120, 112, 116, 124], 4, -1),              # padded images exceed the LDS: generic wide kernels
])
def test_backward_kind_reads_the_shape_plan(hid, E, kind):
    m = C.desc(dict(hid=hid, E=E, out_act=C.ELU))
    assert _lib.lib().umnn_cc_backward_kind(ctypes.byref(m), E) == kind
    assert _lib.lib().umnn_cc_backward_kind(ctypes.byref(m), E + 1) == -2      # (widths[0] != 1 + E: an error, not a family)
