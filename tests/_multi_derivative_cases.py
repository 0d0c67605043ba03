"""Truth, cotangents and bounds of the multi-output derivative tests: tests/test_multi_derivative_cpu.py (no GPU) and
tests/test_gpu_multi_derivative.py (umnn_cc_backward_multi_fx itself, the operator and the module).

The cases, inputs, kink rule (GUARD = 1e-5), floor and outer bound are those of tests/_multi_coverage_cases.py, untouched.  New here
is the cotangent g_fx [B, d, K] of f_x[q][k] = f_k(x_q; h_q), drawn in float64 from a generator of its own and rounded to float32, and
the truth that goes with it: the row problem in torch on the float32-rounded weights, inputs and tables,

    d_h, d_theta = autograd of  sum(F g) + sum(f(x) g_fx)
    d_x          = sum_k g_k f_k(x)  (the Leibniz term the operator defines)  +  autograd in x of  sum(f(x) g_fx)  alone
    d_x0         = -sum_k g_k f_k(x0)

in float64 (the truth) and in float32 (the same arithmetic at the kernels' precision): E32 = the error of the float32 run against the
float64 one, floored at 2^-22.  A kernel output must be within M x E32 of the truth, never above 1e-5 (`bound`): U.rel_err for d_x
and d_x0, U.scaled_err for d_h and each parameter tensor.  M starts at the project's M_GRAD = 8; an output that needs more gets twice
its largest measured ratio, with the sum responsible named, in M_OF (profiles/multi_derivative/README.md holds the measured ratios).
`zero_g`: the same with g = 0, the cotangent of a loss that reads f_x alone."""
import copy
import types

import torch

from tests import _multi_coverage_cases as C
from tests import _multi_output_cases as M
from umnn_amd.quadrature import compute_cc_weights

M_OF = {}            # output -> M where the measured ratio asks for more than C.M_GRAD (none does: profiles/multi_derivative/README.md)
_GFX, _TRUTH = {}, {}


def gfx_of(c):
    """g_fx [B, d, K]: float64 CPU tensor holding float32 values, from a generator of its own; computed once per shape, never modified"""
    key = (c["B"], c["d"], c["K"])
    if key not in _GFX:
        gen = torch.Generator().manual_seed(90001 + 53 * c["B"] + 19 * c["d"] + 1013 * c["K"])
        _GFX[key] = torch.randn(c["B"], c["d"], c["K"], generator=gen, dtype=torch.float64).float().double()
    return _GFX[key]


def quadrature_fx(f, params, x0, x, h, g, gfx, n, inv_f=False, dtype=torch.float64, chunk=4096):
    """`C.quadrature` with the cotangent gfx [R, K] of f(x) on top of g [R, K] -> namespace of numpy arrays fx [R, K]; dx0, dx [R]; dh [R, E];
    dxfx [R]: the autograd part of dx alone; dtheta: one array per entry of params."""
    w, s = (t.reshape(-1).to(dtype) for t in compute_cc_weights(n))
    x, h, g, gfx = x.to(dtype), h.to(dtype), g.to(dtype), gfx.to(dtype)
    x0 = torch.zeros_like(x) if x0 is None else x0.to(dtype)
    assert h.shape[1] > 0
    acc = [torch.zeros_like(p) for p in params]
    out = {k: [] for k in ("fx", "dx0", "dx", "dxfx", "dh")}
    for lo in range(0, x.shape[0], chunk):
        xa, x0a, ga, gfa = x[lo:lo + chunk], x0[lo:lo + chunk], g[lo:lo + chunk], gfx[lo:lo + chunk]
        ha = h[lo:lo + chunk].detach().requires_grad_(True)
        xr = xa.detach().clone().requires_grad_(True)          # the x of f(x) alone: the nodes below are built on xa
        r = xa.shape[0]
        t = x0a[:, None] + (xa - x0a)[:, None] * (s[None, :] + 1) / 2
        rows = torch.cat((t[:, :, None], ha[:, None, :].expand(r, n + 1, ha.shape[1])), 2).reshape(r * (n + 1), -1)
        v = f(rows).view(r, n + 1, -1)
        F = ((1 / v if inv_f else v) * w[None, :, None]).sum(1) * ((xa - x0a) / 2)[:, None]
        fxr = f(torch.cat((xr[:, None], ha), 1))
        gr = torch.autograd.grad((F * ga).sum() + (fxr * gfa).sum(), list(params) + [ha, xr])
        for a, b in zip(acc, gr):
            a += b
        with torch.no_grad():
            fx, fx0 = f(torch.cat((xa[:, None], ha), 1)), f(torch.cat((x0a[:, None], ha), 1))
        out["fx"].append(fx); out["dh"].append(gr[len(params)]); out["dxfx"].append(gr[len(params) + 1])
        out["dx"].append((ga * fx).sum(1) + gr[len(params) + 1]); out["dx0"].append(-(ga * fx0).sum(1))
    res = {k: torch.cat(v).detach().numpy() for k, v in out.items()}
    return types.SimpleNamespace(dtheta=[a.numpy() for a in acc], **res)


def case_quadrature_fx(c, i, dtype, zero_g=False, gfx=None, rows=None):
    """`quadrature_fx` of a case's inputs `i` on its float32-rounded weights (all integrals, or the integrals `rows`)"""
    seq = copy.deepcopy(i.net.net).to(dtype)
    x, h = C.rows_of(i.x, i.h, c["d"])
    x0 = None if i.x0 is None else i.x0.reshape(-1)
    g = i.g.reshape(-1, c["K"])
    g = torch.zeros_like(g) if zero_g else g
    gfx = (gfx_of(c) if gfx is None else gfx).reshape(-1, c["K"])
    if rows is not None:
        x, h, g, gfx, x0 = x[rows], h[rows], g[rows], gfx[rows], (None if x0 is None else x0[rows])
    return quadrature_fx(seq, list(seq.parameters()), x0, x, h, g, gfx, c["n"], c["inv_f"], dtype)


def errors(got, ref):
    """`C.errors` of the gradient outputs (dtheta a list, one per parameter tensor)"""
    return C.errors(types.SimpleNamespace(dx0=getattr(got, "dx0", None), dx=getattr(got, "dx", None), dh=getattr(got, "dh", None),
                                          dtheta=getattr(got, "dtheta", None)), ref)


def truth(c, zero_g=False):
    """-> namespace(t: the float64 truth, t32: the float32 run, E32: {output: max(error of t32 against t, 2^-22)}).  Computed once per
    (input set, inv_f, zero_g) and shared; callers must not modify it."""
    key = C._input_key(c) + (c["inv_f"], zero_g)
    if key not in _TRUTH:
        i = C.inputs(c)
        t, t32 = (case_quadrature_fx(c, i, dt, zero_g) for dt in (torch.float64, torch.float32))
        E32 = {k: ([max(v, C.FLOOR) for v in e] if isinstance(e, list) else max(e, C.FLOOR)) for k, e in errors(t32, t).items()}
        _TRUTH[key] = types.SimpleNamespace(t=t, t32=t32, E32=E32)
    return _TRUTH[key]


def bound(E32, name):
    """the rel_err / scaled_err bound of one output (one parameter tensor of dtheta): M x E32, never above 1e-5"""
    return min(M_OF.get(name, C.M_GRAD) * E32, C.OUTER)


# ---- the nets and flag cases of the device test: every family and every pass list -----------------------------------------------
NETS = {(2, 8): ([20, 31, 9], [31] * 5), (4, 13): ([51, 40, 33], [40] * 7), (4, 16): ([63, 52, 60], [52, 63, 56, 60, 63, 55]),
        (7, 26): ([103], [103, 64], [80, 103, 70], [103] * 4), (8, 32): ([127], [127, 104])}
NET_CASES = [next(c for c in C.CASES if c["part"] == 1 and c["hid"] == list(hid)) for fam, nets in NETS.items() for hid in nets]
FLAG_CASES = [C.FLAG_CASES[fam, flag] for fam in C.REPS for flag in ("no-x0", "inv_f", "relu", "sigmoid", "K16")]
DEVICE_CASES = NET_CASES + FLAG_CASES


def fx_name(name):
    """the name the library notes for the g_fx build of a backward pass"""
    return name[:-1] + ",FX=1>"


# ---- float64 model of MonotonicNN.forward_with_derivative -------------------------------------------------------------------------
def mono64(m64, x, h, quadrature64):
    """(y, log dy/dx) of a float64 copy `m64` of a MonotonicNN in plain torch.  dy/dx is the defined one, exp(s) f(x; h), and the
    gradient of y in x is the Leibniz term the operator defines (not autograd through the nodes): the nodes are built on x.detach()
    and (x - x.detach()) f(x.detach(); h).detach() carries f(x) to x."""
    out = m64.net(h)
    K = m64.n_out
    off, ls = (out[:, [0]], out[:, [1]]) if K == 1 else (out[:, :K], out[:, K:])
    xd = x.detach()
    F = quadrature64(m64.integrand, torch.zeros_like(xd), xd, h, m64.nb_steps)
    F = F + (x - xd) * m64.integrand(xd, h).detach()
    return torch.exp(ls) * F + off, ls + torch.log(m64.integrand(x, h))


def operator_truth(net, x, h, g, gfx, nb_steps):
    """float64 truth of (F, f_x) = IntegralWithDerivative(0, x, net, ., h, nb_steps) and of the gradients of sum(F g) + sum(f_x gfx)
    -> (F, f_x, dx, dh, [dparams]) in numpy: dx = the Leibniz term sum_k g_k f_k(x) + autograd in x of sum(f(x) gfx) alone."""
    net64 = copy.deepcopy(net).double()
    x64, h64 = x.double().clone().requires_grad_(), h.double().clone().requires_grad_()
    xd = x64.detach()
    F = M.quadrature64(net64, torch.zeros_like(xd), xd, h64, nb_steps)
    fx = net64(x64, h64)
    ((F * g.double()).sum() + (fx * gfx.double()).sum()).backward()
    dx = x64.grad + (fx.detach() * g.double()).sum(1, keepdim=True)
    return F.detach().numpy(), fx.detach().numpy(), dx.numpy(), h64.grad.numpy(), [p.grad.numpy() for p in net64.parameters()]
