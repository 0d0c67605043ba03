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
