"""umnn_cc_backward_plan_name against what a backward call really does, for the smallest cases of tests/_bwd_plan_cases.py: the name the
query gives before the call is the name the call notes, and the call counts the launches it counted before the launch plan moved
into csrc/cc_bwd_plan.h."""
import ctypes

import pytest
import torch

from tests import _bwd_plan_cases as C
from umnn_amd import _lib

# umnn_launch_count() delta of one call (main pass or passes, d_h, d_theta reduction), recorded once on the build before the plan
# header existed (tools/path_identity.py run, profiles/bwd_plan/): two fp32 passes for the 100-80-70 net, one main launch elsewhere
LAUNCHES_BEFORE = {c["id"]: 3 for c in C.GPU_CASES}
LAUNCHES_BEFORE["fp32-pad26"] = 4


@pytest.mark.gpu
@pytest.mark.parametrize("c", C.GPU_CASES, ids=[c["id"] for c in C.GPU_CASES])
def test_the_call_runs_what_the_plan_names(c):
    lib = _lib.lib()
    dev = torch.device("cuda:0")
    m = C.desc(c)
    with _lib.options(**c["options"]), torch.cuda.device(dev):
        planned = lib.umnn_cc_backward_plan_name(ctypes.byref(m), c["B"], c["d"], c["E"], c["n"], c["flags"]).decode()
    before = lib.umnn_launch_count()
    out = C.run(c, dev)
    torch.cuda.synchronize()
    assert planned == c["name"]
    assert lib.umnn_last_kernel_name_of(_lib.PROF_BACKWARD).decode() == planned
    assert lib.umnn_launch_count() - before == LAUNCHES_BEFORE[c["id"]]
    assert all(torch.isfinite(t).all() for t in out if t is not None)
