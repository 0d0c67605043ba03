"""Cases and float64 truth of the curve-gradient tests (tests/test_curve_grad_cpu.py, tests/test_gpu_curve_grad.py): the backward of
``MonotonicNN.forward_curve`` / ``cumulative_incidence`` / ``IntegralCurve`` / ``cumulate`` with ``backward="hip"``.

Cases are those of tests/_curve_cases.py (its seven ``CASES``, ``X0_CASE`` / ``x0_of()``, ``P2_BASE``, ``CIF_CASE``), with row 0 moved
onto the lower limit: x[0] = 0 for the model cases, x[0] = x0[0] for the operator case -- a row of zero span is an ordinary row of the
backward (no division by the span anywhere).  The ragged case repeats the 37 rows of ``P2_BASE`` (unmodified) to ``ragged_rows(cus)``
= cus * 4 * 16 + 5 rows: more 16-row groups than the backward has persistent waves, so a wave walks more than one, and a last group of
five rows.

Truth is float64 torch, ``_curve_cases.curve64`` plus the float64 model, and the loss

    sum(y * G1) + sum(dy/dt * G2) + sum(t * G3)          (operator: C and f in place of y and dy/dt)

with fixed random G, so that all three cotangent routes of the backward are live; the gradients in x, h and every parameter (x0
too, through the operator) come from autograd.  Criterion: ``_util.scaled_err`` <= TOL = 1e-5 per tensor (dx, dh, each parameter),
the project's bound for the multi-output backward (``_multi_output_cases.TOL``); every case asserts its kink margin >=
MIN_MARGIN = 1e-6 and no row is excluded.  The float32 ATen composition under autograd is itself within dx 1.7e-7, dh 3.0e-7, a
single parameter 6.5e-7 of this truth over the seven cases (test_curve_grad_cpu prints the figures), which leaves the kernels about
15x room."""
import copy
import functools
from collections import namedtuple

import torch

from tests import _curve_cases as C

TOL = C.TOL
MIN_MARGIN = C.MIN_MARGIN
HIP_CASES = [i for i, c in enumerate(C.CASES) if c.K <= 16]

GradTruth = namedtuple("GradTruth", "dx0 dx dh dparams margin")      # numpy; dparams {name: array} in named_parameters() order


def cotangents(B, n, K):
    """(G1 [B, n+1, K], G2 [B, n+1, K], G3 [B, n+1]) float64, fixed."""
    g = torch.Generator().manual_seed(11)
    return (torch.randn(B, n + 1, K, generator=g, dtype=torch.float64), torch.randn(B, n + 1, K, generator=g, dtype=torch.float64),
            torch.randn(B, n + 1, generator=g, dtype=torch.float64))


def loss_of(out, G):
    """The loss of the docstring for out = (t, y, dy) or (t, C, f) and G = ``cotangents`` in out's dtype and device."""
    t, y, dy = out
    return (y * G[0]).sum() + (dy * G[1]).sum() + (t * G[2]).sum()


def on(G, like):
    return tuple(g.to(device=like.device, dtype=like.dtype) for g in G)


def build(i):
    """CASES[i] with row 0 on the lower limit -> (MonotonicNN fp32 on the CPU, x, h)."""
    model, x, h = C.build(C.CASES[i])
    x = x.clone()
    x[0] = 0.
    return model, x, h


def model64(model, x, h):
    """(t, y, dy/dt) of a MonotonicNN in float64, differentiable: ``_curve_cases.truth``'s forward."""
    K = model.n_out
    t, Cv, f = C.curve64(model.integrand, torch.zeros_like(x), x, h, model.nb_steps)
    out = model.net(h)
    o, sc = out[:, :K].unsqueeze(1), torch.exp(out[:, K:]).unsqueeze(1)
    return t, sc * Cv + o, sc * f


def model_truth(model, x, h, G=None):
    m64 = copy.deepcopy(model).double()
    x64, h64 = x.double().clone().requires_grad_(), h.double().clone().requires_grad_()
    G = cotangents(x.shape[0], model.nb_steps, model.n_out) if G is None else G
    names = [n for n, _ in m64.named_parameters()]
    grads = torch.autograd.grad(loss_of(model64(m64, x64, h64), G), [x64, h64] + list(m64.parameters()))
    return GradTruth(None, grads[0].numpy(), grads[1].numpy(), {n: g.numpy() for n, g in zip(names, grads[2:])},
                     C.M.margin(model.integrand, None, x, h, model.nb_steps))


@functools.lru_cache(maxsize=None)
def case_truth(i):
    """Truth of ``build(i)``, computed once and shared (callers must not modify it)."""
    return model_truth(*build(i))


def x0_case():
    """-> (integrand fp32 on the CPU, x0, x, h, nb_steps): X0_CASE through the operator, row 0 with x = x0."""
    net, x, h, _ = C.M.build(C.X0_CASE)
    x0 = C.x0_of()
    x = x.clone()
    x[0] = x0[0]
    return net, x0, x, h, C.X0_CASE.nb_steps


@functools.lru_cache(maxsize=None)
def x0_truth():
    net, x0, x, h, n = x0_case()
    net64 = copy.deepcopy(net).double()
    x064, x64, h64 = (v.double().clone().requires_grad_() for v in (x0, x, h))
    G = cotangents(x.shape[0], n, C.X0_CASE.K)
    names = [k for k, _ in net64.named_parameters()]
    grads = torch.autograd.grad(loss_of(C.curve64(net64, x064, x64, h64, n), G), [x064, x64, h64] + list(net64.parameters()))
    return GradTruth(grads[0].numpy(), grads[1].numpy(), grads[2].numpy(), {k: g.numpy() for k, g in zip(names, grads[3:])},
                     C.M.margin(net, x0, x, h, n))


def ragged_rows(cus):
    return cus * 4 * 16 + 5


def ragged_case(cus):
    """-> (model, x, h, index [B] of the base row each row repeats, G of the repeated batch: the base rows' cotangents repeated)."""
    model, x, h = C.build(C.P2_BASE)
    idx = torch.arange(ragged_rows(cus)) % C.P2_BASE.B
    G = tuple(g[idx].contiguous() for g in cotangents(C.P2_BASE.B, C.P2_BASE.nb_steps, C.P2_BASE.K))
    return model, x[idx].contiguous(), h[idx].contiguous(), idx, G


def cif_case():
    model, x, h = C.build(C.CIF_CASE)
    return model, x.abs() + 0.5, h


@functools.lru_cache(maxsize=None)
def cif_truth():
    """Gradients of sum(CIF * G) in h and every parameter from the float64 model's own autograd -> (G [B, n+1, K] float64, dh, dparams)."""
    model, x, h = cif_case()
    m64 = copy.deepcopy(model).double()
    h64 = h.double().clone().requires_grad_()
    cif = m64.cumulative_incidence(x.double(), h64, curve=True)[1]
    G = torch.randn(cif.shape, generator=torch.Generator().manual_seed(12), dtype=torch.float64)
    names = [k for k, _ in m64.named_parameters()]
    grads = torch.autograd.grad((cif * G).sum(), [h64] + list(m64.parameters()))
    return G, grads[0].numpy(), {k: g.numpy() for k, g in zip(names, grads[1:])}
