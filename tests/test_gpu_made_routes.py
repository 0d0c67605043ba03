"""Every route of the conditioner that a device call can reach (the ``gpu`` entries of tests/_made_route_cases.py), through ``raw`` on the
smallest conditioner that reaches it: the launches and the kernel that the hand-written route record implies, and the result against
the fp32 ``F.linear`` chain within the bounds of tests/test_gpu_made.py (2e-5 of the largest entry for fp32 output, 6e-3 for bf16)."""
import contextlib
import dataclasses

import pytest
import torch

from tests import _made_route_cases as C

pytestmark = pytest.mark.gpu

GPU_CASES = [c for c in C.CASES if c["gpu"] is not None]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


@pytest.mark.parametrize("out_dtype", [None, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("case", GPU_CASES, ids=[c["id"] for c in GPU_CASES])
def test_route_launches_and_result(dev, case, out_dtype):
    import umnn_amd
    from umnn_amd import _lib, made as M
    g, (name, _, lib_out), rows = case["gpu"], case["expect"], case["rows"]
    spec = g["net"]
    torch.manual_seed(len(case["id"]) + rows)
    if spec[0] == "COND":
        net = M.ConditionnalMADE(spec[1], spec[2], spec[3], spec[4], num_masks=1, natural_ordering=True).to(dev)
        args = [torch.randn(rows, spec[1], device=dev) * 2, torch.randn(rows, spec[2], device=dev)]
    else:
        net = M.MADE(spec[1], spec[2], spec[3], num_masks=1, natural_ordering=True).to(dev)
        args = [torch.randn(rows, spec[1], device=dev) * 2]
    layers = [l for l in net.net if isinstance(l, M.MaskedLinear)]
    assert [(l.in_features, l.out_features) for l in layers] == case["widths"]
    with torch.no_grad():
        for l in layers:
            l.bias.uniform_(-1.0, 1.0)
    if g.get("double"):
        net, args = net.double(), [a.double() for a in args]
    if g.get("frozen"):
        net.requires_grad_(False)
    if "x_dtype" in g:
        args[0] = args[0].to(getattr(torch, g["x_dtype"]))
    if "ctx_dtype" in g:
        args[1] = args[1].to(getattr(torch, g["ctx_dtype"]))
    lib = _lib.lib()
    old = dataclasses.replace(M._OPTIONS)
    try:
        umnn_amd.set_made_fast_path(g.get("fast", True))
        umnn_amd.set_made_fused(g.get("fused_enabled", True), **g.get("fused", {}))
        M._TRAIN_FUSED["enabled"] = g.get("train_fused", True)
        autocast = (lambda: torch.autocast("cuda", dtype=torch.bfloat16)) if g.get("autocast") else contextlib.nullcontext
        n0 = lib.umnn_made_launch_count()
        with (torch.enable_grad() if g.get("grad") else torch.no_grad()), autocast():
            out = net.raw(*args, out_dtype=out_dtype)
        launches, kernel = lib.umnn_made_launch_count() - n0, lib.umnn_last_made_kernel_name().decode()
        umnn_amd.set_made_fast_path(False)
        with torch.no_grad(), autocast():           # (the F.linear chain, under the case's autocast if it has one)
            exact = net.raw(*args)
    finally:
        umnn_amd.set_made_fast_path(old.fast)
        umnn_amd.set_made_fused(old.fused, old.max_rows, old.wide_out, old.hybrid, old.layered)
        M._TRAIN_FUSED["enabled"] = old.train_fused
    assert M._OPTIONS == dataclasses.replace(old, probe=M._OPTIONS.probe), "every switch is back (the one-time probe may have run)"
    count, kernel_name = C.LAUNCHES[name]
    assert launches == count(len(layers), lib_out), (launches, kernel)
    if kernel_name is not None:
        assert kernel_name in kernel
    if out_dtype is None:
        assert (type(out.grad_fn).__name__ == "_MadeTrainChainBackward") == (name == "train")
    assert (out.grad_fn is not None) == bool(g.get("grad") and not g.get("frozen"))
    chain_dtype = torch.float64 if g.get("double") else torch.bfloat16 if g.get("autocast") else torch.float32
    assert out.dtype == (out_dtype or chain_dtype) and exact.dtype == chain_dtype
    assert out.shape == exact.shape == (rows, case["n_out"])
    scale = exact.abs().max().item()
    err = (out.detach().double() - exact.double()).abs().max().item()
    if name == "split" and out_dtype is None:
        # three bf16 products accumulated in fp32 do not round like the fp32 GEMM: bit equality would mean the F.linear chain ran
        assert not torch.equal(out, exact), "split + GEMM must not be the F.linear chain"
    print(f"{case['id']}: {name}, {launches} launches, |out - fp32 chain| = {err / scale:.2e} of the largest entry")
    assert scale > 0 and err <= (2e-5 if out_dtype is None else 6e-3) * scale
