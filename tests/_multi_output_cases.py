"""Cases and float64 truth of the multi-output quadrature tests (tests/test_multi_output_cpu.py, tests/test_gpu_multi_output.py).

Truth is a plain-torch float64 quadrature of the same weights on the CPU, (x - x0)/2 * sum_j w_j f_k(t_j) with
``compute_cc_weights``, gradients by autograd -- except the gradient for the LIMITS, which the operator defines (like the
reference, ParallelNeuralIntegral.py:110-123, and like every single-output test here) as the Leibniz terms dx = sum_k g_k f_k(x),
dx0 = -sum_k g_k f_k(x0): autograd through the nodes differs from them by the quadrature error (2e-3 at the 7 steps of case 0), so
their truth is that formula in float64, at the same tolerance.  Tolerance 1e-5: values with ``rel_err``, gradients with ``scaled_err``.  The
float32 ATen composition alone is within 3.1e-7 (values) and 2.4e-7 (gradients) of float64 on these cases; the kernels differ from
it by summation order and by ``__expf`` in the output activation, so 1e-5 leaves about 30x room and is 10x tighter than the
project-wide 1e-4.  Every case's kink margin (``_util.kink_margin``, float64) is asserted >= 1e-6 and no row is excluded.

Construction: ``torch.manual_seed(seed)``, then the ``nn.Linear`` layers in order with default init; a ``torch.Generator`` seeded
``100 + seed`` draws x = randn(B,1) * 2, h = randn(B, in_d - 1), g = randn(B, K), in that order."""
import functools
from collections import namedtuple

import numpy as np
import torch
import torch.nn as nn

from oracle import cc_oracle as O
from tests import _util as U
from umnn_amd.quadrature import compute_cc_weights

TOL = 1e-5
MIN_MARGIN = 1e-6

Case = namedtuple("Case", "seed B in_d hidden K nb_steps act")
CASES = [
    Case(0, 37, 3, [20, 33, 17], 2, 7, "ReLU"),
    Case(1, 37, 3, [20, 33, 17], 5, 20, "LeakyReLU"),
    Case(2, 19, 2, [100, 100, 100], 16, 20, "ReLU"),
    Case(3, 19, 4, [127, 50], 3, 50, "ReLU"),
    Case(4, 33, 3, [50, 50, 50, 50], 17, 20, "LeakyReLU"),
]


class IntegrandNN(nn.Module):
    """Linear -> act -> ... -> Linear -> ELU, + 1 outside: the module tree of ``umnn_amd.IntegrandNN`` with either hidden
    activation (``mlp_spec`` recognises foreign classes by this class name and their structure)."""

    def __init__(self, sizes, act, out="ELU"):
        super().__init__()
        layers = []
        for i in range(len(sizes) - 1):
            layers.append(nn.Linear(sizes[i], sizes[i + 1]))
            if i < len(sizes) - 2:
                layers.append(nn.ReLU() if act == "ReLU" else nn.LeakyReLU())
            else:
                layers.append(nn.ELU())
        self.net = nn.Sequential(*layers)

    def forward(self, x, h):
        return self.net(torch.cat((x, h), 1)) + 1.


def build(case):
    """-> (integrand fp32 on CPU, x, h, g)."""
    torch.manual_seed(case.seed)
    net = IntegrandNN([case.in_d] + list(case.hidden) + [case.K], case.act)
    gen = torch.Generator().manual_seed(100 + case.seed)
    x = torch.randn(case.B, 1, generator=gen) * 2
    h = torch.randn(case.B, case.in_d - 1, generator=gen)
    g = torch.randn(case.B, case.K, generator=gen)
    return net, x, h, g


def quadrature64(f, x0, x, h, nb_steps, inv_f=False):
    """(x - x0)/2 * sum_j w_j f_k(t_j) in the dtype of x (float64 for the truth), differentiable.  f(t [N,1], h [N,E]) -> [N,K]."""
    w, s = compute_cc_weights(nb_steps)
    w = torch.as_tensor(np.asarray(w, np.float64).reshape(-1), dtype=x.dtype)
    s = torch.as_tensor(np.asarray(s, np.float64).reshape(-1), dtype=x.dtype)
    total = 0
    for j in range(nb_steps + 1):
        t = x0 + (x - x0) * (s[j] + 1) / 2
        v = f(t, h)
        total = total + w[j] * (1 / v if inv_f else v)
    return total * (x - x0) / 2


Truth = namedtuple("Truth", "F dx dh dparams margin")


def truth(net, x, h, g, nb_steps, x0=None, inv_f=False):
    """float64 values and gradients of sum(F * g) -> Truth (numpy); dparams in parameters() order."""
    net64 = _double(net)
    x64 = x.double().clone().requires_grad_()
    h64 = h.double().clone().requires_grad_()
    x064 = torch.zeros_like(x64) if x0 is None else x0.double()
    F = quadrature64(net64, x064, x64, h64, nb_steps, inv_f)
    (F * g.double()).sum().backward()
    with torch.no_grad():
        dx = (net64(x64, h64) * g.double()).sum(1, keepdim=True)          # the Leibniz term (f itself under inv_f, as the kernels)
    return Truth(F.detach().numpy(), dx.numpy(), h64.grad.numpy(), [p.grad.numpy() for p in net64.parameters()],
                 margin(net, x0, x, h, nb_steps))


def _double(net):
    import copy
    return copy.deepcopy(net).double()


def margin(net, x0, x, h, nb_steps):
    lins = [m for m in net.net if isinstance(m, nn.Linear)]
    leaky = any(isinstance(m, nn.LeakyReLU) for m in net.net)
    onet = O.Net([l.weight.detach().double().numpy() for l in lins], [l.bias.detach().double().numpy() for l in lins],
                 O.LEAKY if leaky else O.RELU, O.ELU1)
    x0n = np.zeros_like(x.numpy()) if x0 is None else x0.numpy()
    return U.kink_margin(onet, x0n, x.numpy(), h.numpy(), nb_steps)


@functools.lru_cache(maxsize=None)
def case_truth(i, inv_f=False):
    """Truth of CASES[i], computed once and shared (callers must not modify it)."""
    net, x, h, g = build(CASES[i])
    return truth(net, x, h, g, CASES[i].nb_steps, inv_f=inv_f)
