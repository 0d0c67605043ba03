"""umnn_cc_launch_plan against what a call really does, for the GPU cases of tests/_fwd_plan_cases.py (the smallest shapes at which
each rule of csrc/cc_fwd_plan.h can go wrong): the name the query gives before the call is the name the call notes, the call is one
launch, and its outputs are finite and right -- the forward against the numpy oracle at the forward parity tolerance of
tests/test_gpu_forward.py, the search and the solves by sending their x back through the float64 oracle's forward map, at the same
tolerance on the target."""
import ctypes

import numpy as np
import pytest
import torch

from oracle import cc_oracle as O
from tests import _fwd_plan_cases as C
from tests import _util as U
from tests._bracket_truth import oracle_net
from tests.test_gpu_forward import TOL
from umnn_amd import _lib


def _check_forward(c, out):
    net, x, h, _ = C.inputs(c)
    net, x, h = oracle_net(net), x.numpy(), h.numpy()
    net = O.Net([W.astype(np.float32) for W in net.Ws], [b.astype(np.float32) for b in net.bs], net.hidden_act, net.out_act)
    F, fx, fx0 = (t.cpu().numpy() for t in out)
    assert U.rel_err(F, O.integrate_parallel(net, np.zeros_like(x), x, h, c["n"])) < TOL
    assert U.rel_err(fx, O.integrand(net, x, h)) < TOL
    assert U.rel_err(fx0, O.integrand(net, np.zeros_like(x), h)) < TOL


def _check_inverse(c, out):
    """exp(scaling_j) (h_0j + int_0^x f) = target for every row whose x is inside the bracket [-50, 50]"""
    net, target, h, scaling = C.inputs(c)
    net64 = oracle_net(net)
    target, h, scaling = target.double().numpy(), h.double().numpy(), scaling.double().numpy()
    B, d = target.shape
    x = out[0].cpu().double().numpy()
    cols = slice(None) if c["kind"] == C.SOLVE_BLOCK else slice(0, 1)
    if c["kind"] != C.SOLVE_BLOCK:
        full = np.zeros_like(target)
        full[:, 0] = x
        x = full
    G = np.exp(scaling) * (h[:, :d] + O.integrate_parallel(net64, np.zeros_like(x), x, h, c["n"]))
    inside = np.abs(x[:, cols]) < 50.0
    assert inside.mean() > 0.5
    err = np.abs(G - target)[:, cols] / np.maximum(np.abs(target[:, cols]), 1.0)
    assert err[inside].max() < TOL


@pytest.mark.gpu
@pytest.mark.parametrize("c", C.GPU_CASES, ids=[c["id"] for c in C.GPU_CASES])
def test_the_call_runs_what_the_plan_names(c):
    lib = _lib.lib()
    dev = torch.device("cuda:0")
    m = C.desc(c)
    info = _lib.LaunchPlanInfo()
    with _lib.options(**c["options"]), torch.cuda.device(dev):
        assert lib.umnn_cc_launch_plan(ctypes.byref(m), c["kind"], c["B"], c["d"], c["E"], c["n"], c["flags"], ctypes.byref(info)) == 0
    before = lib.umnn_launch_count()
    out = C.run(c, dev)
    torch.cuda.synchronize()
    assert info.name.decode() == c["name"]
    assert lib.umnn_last_kernel_name().decode() == c["name"]
    assert lib.umnn_launch_count() - before == 1
    assert (info.P, info.ns, info.waves_per_block, info.blocks, info.fallback) == (c["P"], c["ns"], c["waves"], c["blocks"], c["fallback"])
    assert all(torch.isfinite(t).all() for t in out)
    (_check_forward if c["kind"] == C.FORWARD else _check_inverse)(c, out)
