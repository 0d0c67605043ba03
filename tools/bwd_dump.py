#!/usr/bin/env python
"""Run the quadrature backward on fixed seeded inputs and save every output (A/B of two library builds: UMNN_CC_LIB=... python
tools/bwd_dump.py out.pt ; python tools/bwd_dump.py --compare a.pt b.pt).  Three case lists:

    bf16      four nets through integral.hip_backward under the default options (the bf16-piece families);
    fp32      every case of tests/_bwd_coverage_cases.CASES whose expected kernel name starts with "cc_bwd<" (the fp32-MFMA passes
              of cc_backward.hip: every variant, flag, node-range split and finishing kernel), through umnn_cc_backward_io under the
              case's own options, on the case's own net and inputs;
    multi     every part-1 and part-2 case of tests/_multi_coverage_cases.CASES (every family and backward pass of cc_multi.hip, the
              flags), as its B d row problem through integral.hip_forward_multi and integral.hip_backward_multi.

--compare prints one line per tensor of every case: "bit-identical", or the largest difference over the largest magnitude."""
import copy
import ctypes
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

if sys.argv[1] == "--compare":
    A, B = torch.load(sys.argv[2]), torch.load(sys.argv[3])
    assert A.keys() == B.keys(), "the two dumps hold different cases"
    same = total = 0
    for k in A:
        assert A[k].keys() == B[k].keys(), k
        for name, u in A[k].items():
            v = B[k][name]
            total += 1
            if u.shape != v.shape:
                print(k, name, f"shapes differ: {tuple(u.shape)} against {tuple(v.shape)}")
            elif torch.equal(u.view(torch.int32), v.view(torch.int32)):      # (on the bits: NaNs and signed zeros count)
                same += 1
                print(k, name, "bit-identical")
            else:
                print(k, name, f"max diff / max {float((u - v).abs().max()) / max(float(u.abs().max()), 1e-30):.3e}")
    print(f"{same} of {total} tensors bit-identical")
    sys.exit(0 if same == total else 1)

import umnn_amd  # noqa: E402
from tests import _bwd_coverage_cases as CB  # noqa: E402
from tests import _multi_coverage_cases as CM  # noqa: E402
from umnn_amd import _lib, integral as I  # noqa: E402
from umnn_amd._common import _ptr, _stream  # noqa: E402
from umnn_amd.nets import mlp_spec  # noqa: E402
from umnn_amd.quadrature import device_tables  # noqa: E402

dev = torch.device("cuda:0")
GRADS = ("dx0", "dx", "dh", "dtheta")
out = {}


def keep(names, tensors):
    return {n: t.detach().float().cpu() for n, t in zip(names, tensors) if t is not None}


# ---- bf16: the default families
for (B, d, E, hid, n) in [(257, 63, 30, [50] * 4, 100), (64, 5, 8, [50] * 2, 20), (5, 3, 4, [48, 60, 36], 7), (100, 6, 30, [50] * 3, 50)]:
    torch.manual_seed(B * 7 + d)
    net = umnn_amd.IntegrandNetwork(d, 1 + E, hid, 1).to(dev)
    with torch.no_grad():
        for p_ in net.parameters():
            p_.mul_(1.7)
    x, x0 = torch.randn(B, d, device=dev) * 2, torch.randn(B, d, device=dev) * 0.3
    h, gg, gf = torch.randn(B, E * d, device=dev) * 3, torch.randn(B, d, device=dev), torch.randn(B, d, device=dev)
    out["bf16 " + str((B, d, hid))] = keep(GRADS, I.hip_backward(mlp_spec(net), x0, x, h, gg, gf, n))

# ---- fp32: the fp32-MFMA passes, through the C entry point under each case's options
lib = _lib.lib()
for c in CB.CASES:
    if not c["name"].startswith("cc_bwd<"):
        continue
    i = CB.inputs(c)
    xdt = torch.bfloat16 if c["x_bf16"] else torch.float32
    hdt = torch.bfloat16 if c["h_bf16"] else torch.float32
    to = lambda t, dt: None if t is None else t.to(dt).to(dev).contiguous()      # noqa: E731
    spec = mlp_spec(copy.deepcopy(i.net).to(dev))
    x0, x, h, g, g_fx = to(i.x0, xdt), to(i.x, xdt), to(i.h, hdt), to(i.g, xdt), to(i.g_fx, xdt)
    B, d, E, n = c["B"], c["d"], c["E"], c["n"]
    outs = [torch.zeros_like(x), torch.zeros_like(x), torch.zeros_like(h),
            torch.zeros(sum(l.weight.numel() + l.bias.numel() for l in spec.linears), device=dev)]
    io = None
    if c["x_bf16"] or c["h_bf16"]:
        io = ctypes.byref(_lib.IoDesc(_lib.DTYPE_BF16 if c["x_bf16"] else _lib.DTYPE_F32, _lib.DTYPE_BF16 if c["h_bf16"] else _lib.DTYPE_F32))
    w, s = device_tables(n, dev)
    desc, alive = I._desc(spec)
    with _lib.options(**c["options"]), torch.cuda.device(dev):
        nbytes = int(lib.umnn_cc_backward_workspace_bytes(ctypes.byref(desc), B, d, E))
        assert nbytes > 0, c["id"]
        ws = torch.empty(nbytes, device=dev, dtype=torch.uint8)
        rc = lib.umnn_cc_backward_io(ctypes.byref(desc), io, _ptr(x0), _ptr(x), _ptr(h), _ptr(g), _ptr(g_fx), _ptr(w), _ptr(s), n, B, d, E,
                                     int(c["inv_f"]), *(_ptr(o) for o in outs), ctypes.c_void_p(ws.data_ptr()), nbytes, _stream(dev))
        _lib.check(rc, "umnn_cc_backward_io")
        torch.cuda.synchronize()
    name = lib.umnn_last_kernel_name_of(_lib.PROF_BACKWARD).decode()
    assert name == c["name"], (c["id"], name, c["name"])
    out["fp32 " + c["id"]] = keep(GRADS, outs)

# ---- multi: every family, pass and flag of the multi-output kernels
for c in CM.CASES:
    if c["part"] not in (1, 2):
        continue
    i = CM.inputs(c)
    to = lambda t: None if t is None else t.float().to(dev).contiguous()      # noqa: E731
    spec = mlp_spec(copy.deepcopy(i.net).to(dev))
    x, h = CM.rows_of(i.x, i.h, c["d"])
    x, h, g = to(x[:, None]), to(h), to(i.g.reshape(-1, c["K"]))
    x0 = None if i.x0 is None else to(i.x0.reshape(-1, 1))
    fwd = I.hip_forward_multi(spec, x0, x, h, c["n"], inv_f=c["inv_f"])
    assert lib.umnn_last_kernel_name().decode() == c["fwd"], c["id"]
    bwd = I.hip_backward_multi(spec, x0, x, h, g, c["n"], inv_f=c["inv_f"])
    torch.cuda.synchronize()
    assert lib.umnn_last_kernel_name_of(_lib.PROF_BACKWARD).decode() == c["last"], c["id"]
    out["multi " + c["id"]] = keep(CM.VALUES + GRADS, fwd + bwd)

torch.save(out, sys.argv[1])
print("saved", sys.argv[1], len(out), "cases,", sum(len(v) for v in out.values()), "tensors")
