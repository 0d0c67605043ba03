"""The flows of the sample-with-log-density tests (tests/test_sample_log_prob_cpu.py on the ATen path in float64,
tests/test_gpu_sample_log_prob.py as fp32 copies on the device): nb_flow 1..3 (both parities of the flips between blocks), nb_in 2, 3, 5,
one conditional flow and one with a Sigmoid integrand output.  Built once per process on the CPU and never modified."""
import torch

import umnn_amd

N = 20
B = 6
METHODS = {
    "newton": dict(method="newton", tol=1e-12),
    "newton-progressive": dict(method="newton", tol=1e-12, conditioner="progressive"),
    "jacobi": dict(method="jacobi", tol=1e-12, sweep_tol=0),       # (max_sweeps = d is added per flow)
    "bracket": dict(method="bracket"),
}
#        name            nb_flow  nb_in  cond_in  act_func
FLOWS = [("f1-d2", 1, 2, 0, "ELU"), ("f1-d3", 1, 3, 0, "ELU"), ("f1-d5", 1, 5, 0, "ELU"),
         ("f2-d2", 2, 2, 0, "ELU"), ("f2-d3", 2, 3, 0, "ELU"), ("f2-d5", 2, 5, 0, "ELU"),
         ("f3-d2", 3, 2, 0, "ELU"), ("f3-d3", 3, 3, 0, "ELU"), ("f3-d5", 3, 5, 0, "ELU"),
         ("cond", 2, 3, 2, "ELU"), ("sigmoid", 2, 3, 0, "Sigmoid")]
_cache = {}


def flow(name):
    """(flow, z, context) of a case, built once and left unchanged."""
    if name not in _cache:
        idx = [f[0] for f in FLOWS].index(name)
        _, nb_flow, d, cond_in, act = FLOWS[idx]
        torch.manual_seed(100 + idx)
        m = umnn_amd.UMNNMAFFlow(nb_flow=nb_flow, nb_in=d, hidden_derivative=[24, 24], hidden_embedding=[16, 16], embedding_s=4,
                                 nb_steps=N, solver="CCParallel", cond_in=cond_in, act_func=act).double().eval()
        with torch.no_grad():
            for blk in m.nets:
                blk.scaling.copy_(0.3 * torch.randn(d, dtype=torch.float64))       # (a zero scaling would hide a dropped s_i)
        z = torch.randn(B, d, dtype=torch.float64)
        ctx = torch.randn(B, cond_in, dtype=torch.float64) if cond_in else None
        _cache[name] = (m, z, ctx)
    return _cache[name]


def opts(method, d):
    o = dict(METHODS[method])
    if o["method"] == "jacobi":
        o["max_sweeps"] = d
    return o


def check_one_x(obj, nb_flow, z, ctx, o):
    """``obj.invert`` (a UMNNMAFFlow of ``nb_flow`` blocks, or a single UMNNMAF: ``nb_flow`` None) returns ONE x whatever else is asked
    for, in exactly the documented shapes: x, (x, log_jac), and for jacobi (x, info) and (x, info, log_jac) -- info's entries lists over
    the blocks for a flow, the block's own values for a single block."""
    B, d = z.shape
    x = obj.invert(z, context=ctx, **o)
    assert torch.is_tensor(x) and x.shape == (B, d)
    out = obj.invert(z, context=ctx, return_log_jac=True, **o)
    assert type(out) is tuple and len(out) == 2 and torch.equal(out[0], x)
    assert torch.is_tensor(out[1]) and out[1].shape == (B,)
    if o["method"] != "jacobi":
        return
    with_info = obj.invert(z, context=ctx, return_info=True, **o)
    both = obj.invert(z, context=ctx, return_info=True, return_log_jac=True, **o)
    assert type(with_info) is tuple and len(with_info) == 2 and type(both) is tuple and len(both) == 3
    assert torch.equal(with_info[0], x) and torch.equal(both[0], x) and torch.equal(both[2], out[1])
    for info in (with_info[1], both[1]):
        assert type(info) is dict and list(info) == ["sweeps", "converged", "status", "max_evals"]
        per_block = list(zip(*(info[k] for k in info))) if nb_flow is not None else [tuple(info.values())]
        if nb_flow is not None:
            assert all(type(v) is list and len(v) == nb_flow for v in info.values())
        for sweeps, converged, status, max_evals in per_block:
            assert type(sweeps) is int and sweeps == o["max_sweeps"] and type(converged) is bool
            assert torch.is_tensor(status) and status.shape == (B, d) and status.dtype == torch.int32
            assert type(max_evals) is list and len(max_evals) == sweeps and all(type(e) is int for e in max_evals)


def composed(m, z, ctx, o):
    """The flow's ``invert(..., return_log_jac=True)`` by hand from the blocks' public ``invert`` -> (x, sum of the blocks' log_jac)."""
    z, lj = torch.flip(z, [1]), 0.
    for i in reversed(range(len(m.nets))):
        z, lj_blk = m.nets[i].invert(torch.flip(z, [1]), context=ctx, return_log_jac=True, **o)
        lj = lj + lj_blk
    return z, lj


def lj_magnitude(truth, x, ctx):
    """sum over blocks and dimensions of |log_jac| at x [B], from the float64 CPU flow ``truth``: what the rounding of a sum of these terms
    is relative to, in whatever order they are added."""
    xi, total = x.detach().cpu().double(), 0.
    with torch.no_grad():
        for blk in truth.nets:
            zz, lj = blk._transform(xi, ctx, want_jac=True)
            total = total + lj.abs().sum(1)
            xi = torch.flip(zz, [1])
    return total
