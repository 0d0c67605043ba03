"""Cases and float64 truth of the weighted-sum inverse tests (tests/test_inverse_sum_cpu.py, tests/test_gpu_inverse_sum.py).

Cases 0..4 are ``_multi_output_cases.CASES`` (families (4,13), (7,26), (8,32), both hidden activations, K = 17); cases 5..7 are built
the same way: hidden [24, 31] with K = 4 (family (2,8)), hidden [63, 40] with K = 7 (family (4,16)), and case 1's net at B = 150
(several workgroups, a partial last tile).

Truth: the map G(x) = (sum_k coef_k F_k(x), sum_k coef_k f_k(x)) is a plain-torch float64 quadrature of the same weights
(``_multi_output_cases.quadrature64``), inverted by ``_inverse_truth.solve64``; ``_inverse_truth.newton64`` restates the kernel's
iteration for the evaluation counts.  Neither shares code with ``umnn_amd.integral.newton_solve`` or the kernels.

Value data: coef = rand(B,K) * 2 from a generator seeded 200 + seed, column 0 set to zero; the target is sum_k coef_k F_k(x) at the
case's own x in float64, rounded to float32 (what every run is given), so the truth is x up to that rounding.
Gradient data: coef = 0.5 + rand(B,K) from a generator seeded 300 + seed, then g_x = randn(B,1) from the same generator; the target is
formed the same way.  Gradient truth, with D = sum_k coef_k f_k(x*):  g_t = g_x / D,  g_coef = -g_t F_k(x*),  and (d_h, d_theta) of
``_multi_output_cases.truth`` at upper limit x* for the cotangent -g_t coef.

Bounds.  Values, per row: |x^ - x*| D(x*) <= (1e-5 + tol) max(1, |t|) -- the solver's own stop bound tol max(1, |t|) on the residual plus
the 1e-5 forward tolerance of the multi-output tests, both in units of the target.  Gradients: 1e-5 ``scaled_err``, the multi-output
tests' own tolerance."""
import functools
from collections import namedtuple

import numpy as np
import torch

from tests import _inverse_truth as IT
from tests import _multi_output_cases as M

Case = M.Case
CASES = list(M.CASES) + [
    Case(5, 21, 3, [24, 31], 4, 12, "ReLU"),
    Case(6, 23, 4, [63, 40], 7, 15, "LeakyReLU"),
    Case(1, 150, 3, [20, 33, 17], 5, 20, "LeakyReLU"),
]
FAMILY = {0: (4, 13), 1: (4, 13), 2: (7, 26), 3: (8, 32), 5: (2, 8), 6: (4, 16), 7: (4, 13)}     # case 4 (K = 17) has no kernel
KERNEL_CASES = sorted(FAMILY)
TOL_X, TOL_G = 1e-5, 1e-5
SOLVE_TOL, LO, HI, MAX_ITER = 1e-6, -50., 50., 64


def kernel_name(i):
    return "cc_solve_multi<T=%d,KS=%d>" % FAMILY[i]


def sum_map(net64, h, coef, nb_steps):
    """G(x [B,1] float64 numpy) -> (S, D) [B,1]: the weighted sum of the K integrals and its derivative in x, float64."""
    h64, c64 = torch.as_tensor(np.asarray(h, np.float64)), torch.as_tensor(np.asarray(coef, np.float64))

    def G(x):
        with torch.no_grad():
            x64 = torch.as_tensor(np.asarray(x, np.float64))
            F = M.quadrature64(net64, torch.zeros_like(x64), x64, h64, nb_steps)
            f = net64(x64, h64)
            return (c64 * F).sum(1, keepdim=True).numpy(), (c64 * f).sum(1, keepdim=True).numpy()
    return G


def parts64(net64, x, h, nb_steps):
    """(F_k, f_k) [B,K] float64 numpy at the upper limit x."""
    with torch.no_grad():
        x64, h64 = torch.as_tensor(np.asarray(x, np.float64)), torch.as_tensor(np.asarray(h, np.float64))
        return M.quadrature64(net64, torch.zeros_like(x64), x64, h64, nb_steps).numpy(), net64(x64, h64).numpy()


Data = namedtuple("Data", "net h coef t g_x x_star D F f evals clamped capped G")


def _data(i, grad):
    c = CASES[i]
    net, x, h, _ = M.build(c)
    gen = torch.Generator().manual_seed((300 if grad else 200) + c.seed)
    if grad:
        coef = 0.5 + torch.rand(c.B, c.K, generator=gen)
        g_x = torch.randn(c.B, 1, generator=gen)
    else:
        coef = torch.rand(c.B, c.K, generator=gen) * 2
        coef[:, 0] = 0.
        g_x = None
    net64 = M._double(net)
    G = sum_map(net64, h.numpy(), coef.numpy(), c.nb_steps)
    t = torch.as_tensor(G(x.numpy())[0]).float()                      # what every run is given
    t64 = t.double().numpy()
    x_star = IT.solve64(G, t64, LO, HI)
    _, evals, clamped, capped = IT.newton64(G, t64, LO, HI, SOLVE_TOL, MAX_ITER)
    F, f = parts64(net64, x_star, h.numpy(), c.nb_steps)
    return Data(net, h, coef, t, g_x, x_star, G(x_star)[1], F, f, evals, clamped, capped, G)


@functools.lru_cache(maxsize=None)
def value_data(i):
    """Value data and truth of CASES[i], computed once and shared (callers must not modify it)."""
    return _data(i, False)


@functools.lru_cache(maxsize=None)
def grad_data(i):
    """Gradient data and truth of CASES[i] -> (Data, g_t, g_coef, d_h, [d_params]) in float64 numpy, computed once and shared."""
    d = _data(i, True)
    g_t = d.g_x.double().numpy() / d.D
    cot = torch.as_tensor(-g_t * d.coef.double().numpy())
    T = M.truth(d.net, torch.as_tensor(d.x_star), d.h, cot, CASES[i].nb_steps)
    return d, g_t, -g_t * d.F, T.dh, T.dparams


def value_bound(x_hat, d, tol=SOLVE_TOL):
    """-> (worst row's share of the bound, the per-row pass mask): |x^ - x*| D(x*) <= (1e-5 + tol) max(1, |t|)."""
    err = np.abs(np.asarray(x_hat, np.float64).reshape(-1, 1) - d.x_star) * d.D
    lim = (TOL_X + tol) * np.maximum(1., np.abs(d.t.double().numpy()))
    return float(np.max(err / lim)), err <= lim
