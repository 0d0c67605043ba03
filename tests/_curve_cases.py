"""Cases and float64 truth of the curve tests (tests/test_curve_cpu.py, tests/test_gpu_curve.py): ``MonotonicNN.forward_curve``,
``cumulative_incidence`` and the operator ``IntegralCurve``.

A case is a ``_multi_output_cases.Case``: its integrand, x, h are ``_multi_output_cases.build``'s (x = randn * 2 has both signs, so
ascending and descending grids), placed into a ``MonotonicNN(in_d, hidden, nb_steps, n_out=K)`` whose conditioner is drawn after
``torch.manual_seed(1000 + seed)``.  ``CASES`` = that module's five (n = 7 odd, 20 and 50 even; B = 37 and 19: full tiles plus a
tail; K = 2, 5, 16, 3; K = 17 the ATen fallback; families (4,13), (7,26), (8,32)) and two of this module: hidden [16, 16], K = 1,
n = 8, B = 1 (family (2,8), a single output, a one-row launch) and hidden [60, 60], K = 4, n = 9, B = 33 (family (4,16)).
``p2_case(cus)`` (GPU only): hidden [16, 16], K = 2, n = 7, B = 2 * 4 * cus * 16 + 5 rows -- the P = 2 variant with a ragged last
group --, the 37 rows of a base case repeated (37 is coprime to the tile sizes, so a row landing in another row's place shows;
the kink margin is the base case's).  ``X0_CASE``: CASES[1] with the non-zero lower limit of test_gpu_multi_output (seed 8),
through the operator.

Truth is the same algorithm in float64: the float64 net at the nodes t_j = x0 + (x - x0)(s_j + 1)/2 (s the fp32 table the kernels
read, like ``_multi_output_cases.quadrature64``), the float64 ``cc_cumulative_matrix``, y = exp(s(h)) C + o(h), in torch so that
gradients come from autograd.  Tolerance ``_multi_output_cases.TOL`` = 1e-5 (``rel_err`` values, ``scaled_err`` gradients), kink margin
>= 1e-6 asserted per case, no row excluded.  The float32 ATen composition (``aten_curve`` on the CPU) is itself within
t 1.0e-07, y 6.5e-07, dy/dt 1.9e-07 of this truth over the seven cases (test_curve_cpu prints the figures), so 1e-5 leaves the
kernels -- another summation order, ``__expf`` in the output activation -- about 10x room.

Cumulative incidence (``CIF_CASE``: 4 rows, K = 2, n = 50, float64 on the CPU): the truth is a nested composite rule, 100 panels
(the curve's nodes and their midpoints) of 20-node Clenshaw-Curtis outside and, for every outer node, the cumulated panels plus a
20-node rule inside.  Against it, separate 50-node nested quadratures to each t_i (what a user computes today, 51 x 51 x 51
evaluations per row) are off by 6.4e-06 at most; the curve is held to twice that figure, computed in the test (its own distance,
measured: 6.6e-06).  That tolerance is quadrature error, not arithmetic."""
import copy
import functools
from collections import namedtuple

import numpy as np
import torch

import umnn_amd
from tests import _multi_output_cases as M
from umnn_amd.quadrature import _tables_f64, cc_cumulative_matrix, compute_cc_weights

TOL = M.TOL
MIN_MARGIN = M.MIN_MARGIN
Case = M.Case

CASES = list(M.CASES[:5]) + [
    Case(10, 1, 3, [16, 16], 1, 8, "ReLU"),
    Case(11, 33, 3, [60, 60], 4, 9, "LeakyReLU"),
]
P2_BASE = Case(12, 37, 3, [16, 16], 2, 7, "ReLU")
CIF_CASE = Case(13, 4, 3, [20, 33, 17], 2, 50, "ReLU")
X0_CASE, X0_SEED = M.CASES[1], 8


def build(case):
    """-> (MonotonicNN fp32 on the CPU with the case's integrand, x [B,1], h [B,E])."""
    net, x, h, _ = M.build(case)
    torch.manual_seed(1000 + case.seed)
    model = umnn_amd.MonotonicNN(case.in_d, list(case.hidden), nb_steps=case.nb_steps, n_out=case.K)
    model.integrand = net
    return model, x, h


def p2_rows(cus):
    return 2 * 4 * cus * 16 + 5


def p2_case(cus):
    """-> (model, x, h, index [B] of the base row each row repeats)."""
    model, x, h = build(P2_BASE)
    idx = torch.arange(p2_rows(cus)) % P2_BASE.B
    return model, x[idx].contiguous(), h[idx].contiguous(), idx


def x0_of(case=X0_CASE):
    return torch.randn(case.B, 1, generator=torch.Generator().manual_seed(X0_SEED))


def nodes64(x0, x, nb_steps):
    """[B, n+1] float64, ascending: x0 + (x - x0)(s_j + 1)/2 with the fp32 node table, the last one x itself."""
    _, s = compute_cc_weights(nb_steps)
    u = torch.as_tensor(np.asarray(s, np.float64).reshape(-1)[::-1].copy()) + 1
    t = x0 + (x - x0) * u.view(1, -1) / 2
    return torch.cat((t[:, :-1], x), 1)


def curve64(net64, x0, x, h, nb_steps):
    """(t, C, f) in float64 torch, differentiable: the algorithm of the curve, written out."""
    B, n = x.shape[0], nb_steps
    t = nodes64(x0, x, n)
    f = net64(t.reshape(-1, 1), h.repeat_interleave(n + 1, 0)).view(B, n + 1, -1)
    Q = torch.as_tensor(cc_cumulative_matrix(n)[::-1, ::-1].copy())          # rows and columns ascending
    C = torch.einsum("ij,bjk->bik", Q, f) * ((x - x0) / 2).unsqueeze(2)
    return t, C, f


Truth = namedtuple("Truth", "t y dy dx dh G margin")


def truth(model, x, h):
    """float64 (t, y, dy/dt) of a MonotonicNN, and the gradients in x and h of sum(y * G) for the fixed G it returns."""
    m64 = copy.deepcopy(model).double()
    n = model.nb_steps
    x64, h64 = x.double().clone().requires_grad_(), h.double().clone().requires_grad_()
    t, C, f = curve64(m64.integrand, torch.zeros_like(x64), x64, h64, n)
    out = m64.net(h64)
    K = model.n_out
    o, sc = out[:, :K].unsqueeze(1), torch.exp(out[:, K:]).unsqueeze(1)
    y, dy = sc * C + o, sc * f
    G = torch.randn(y.shape, generator=torch.Generator().manual_seed(7), dtype=torch.float64)
    dx, dh = torch.autograd.grad((y * G).sum(), (x64, h64))
    return Truth(t.detach().numpy(), y.detach().numpy(), dy.detach().numpy(), dx.numpy(), dh.numpy(), G,
                 M.margin(model.integrand, None, x, h, n))


@functools.lru_cache(maxsize=None)
def case_truth(i):
    """Truth of CASES[i], computed once and shared (callers must not modify it)."""
    return truth(*build(CASES[i]))


@functools.lru_cache(maxsize=None)
def p2_truth():
    return truth(*build(P2_BASE))


# ---- cumulative incidence: nested composite truth and the separate quadratures a user runs today -------------------------------
def _cc(fun, a, b, n):
    """int_a^b fun by the n-node Clenshaw-Curtis rule in float64; a, b [...]; fun([..., n+1]) -> [..., n+1, K]  ->  [..., K]."""
    w, s = (torch.as_tensor(v) for v in _tables_f64(n))
    nodes = a.unsqueeze(-1) + (b - a).unsqueeze(-1) * (s + 1) / 2
    return (fun(nodes) * w.view(-1, 1)).sum(-2) * ((b - a) / 2).unsqueeze(-1)


def _row_functions(m64, h_row):
    out = m64.net(h_row.view(1, -1))[0]
    K = out.numel() // 2
    o, sc = out[:K], torch.exp(out[K:])

    def f(t):       # [...] -> [..., K]
        return m64.integrand(t.reshape(-1, 1), h_row.view(1, -1).expand(t.numel(), -1)).view(*t.shape, K)

    return f, o, sc


def cif_composite(m64, x, h, t_nodes, sub=20):
    """CIF at the nodes t_nodes [B, n+1] (ascending from 0) by the nested composite rule of the docstring -> [B, n+1, K]."""
    res = []
    with torch.no_grad():
        for b in range(x.shape[0]):
            f, o, sc = _row_functions(m64, h[b])
            tn = t_nodes[b]
            edges = torch.stack((tn[:-1], (tn[:-1] + tn[1:]) / 2), 1).reshape(-1)
            edges = torch.cat((edges, tn[-1:]))
            lo, hi = edges[:-1], edges[1:]
            cum = torch.cat((torch.zeros(1, o.numel(), dtype=torch.float64), torch.cumsum(_cc(f, lo, hi, sub), 0)))     # int_0^edge f

            def g(s):       # outer integrand at the sub-nodes s [P, sub+1] of the panels
                inner = _cc(f, lo.unsqueeze(1).expand_as(s), s, sub)
                H = sc * (cum[:-1].unsqueeze(1) + inner) + o
                return sc * f(s) * torch.exp(-H.sum(-1, keepdim=True))

            panels = _cc(g, lo, hi, sub)
            cif = torch.cat((torch.zeros(1, o.numel(), dtype=torch.float64), torch.cumsum(panels, 0)))
            res.append(cif[::2])
    return torch.stack(res)


def cif_separate(m64, x, h, t_nodes, n):
    """CIF at the same nodes by a separate n-node quadrature to each, whose integrand takes a separate n-node quadrature per node."""
    res = []
    with torch.no_grad():
        for b in range(x.shape[0]):
            f, o, sc = _row_functions(m64, h[b])
            tn = t_nodes[b]

            def g(s):
                H = sc * _cc(f, torch.zeros_like(s), s, n) + o
                return sc * f(s) * torch.exp(-H.sum(-1, keepdim=True))

            res.append(_cc(g, torch.zeros_like(tn), tn, n))
    return torch.stack(res)
