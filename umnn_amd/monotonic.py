"""MonotonicNN: a scalar function monotone in x, y = exp(s(h)) * int_0^x f(t;h) dt + o(h).

Mirrors models/UMNN/MonotonicNN.py:29-54 (constructor ``MonotonicNN(in_d, hidden_layers, nb_steps=50, dev="cpu")``,
``forward(x, h)`` with x [B,1] and h [B,in_d-1], state_dict keys ``integrand.net.*`` / ``net.*``).  The integral is
the same HIP kernel as the flow's (d = 1, E = in_d-1, ReLU hidden layers).

``inverse(y, h)`` (an extension of this package: the reference has no such method) returns the x with forward(x, h) = y --
quantile functions, inverse-CDF sampling, calibration maps -- by the in-kernel Newton solve, differentiable in y, h and every parameter.
"""
import torch
import torch.nn as nn

from .integral import InverseNeuralIntegral, ParallelNeuralIntegral, _flatten
from .nets import IntegrandNN  # noqa: F401  (re-exported)


class MonotonicNN(nn.Module):
    def __init__(self, in_d, hidden_layers, nb_steps=50, dev="cpu"):
        super().__init__()
        self.integrand = IntegrandNN(in_d, hidden_layers)
        sizes = [in_d - 1] + list(hidden_layers) + [2]      # conditioner -> (offset, log-scale)
        layers = []
        for i in range(len(sizes) - 1):
            layers.append(nn.Linear(sizes[i], sizes[i + 1]))
            if i < len(sizes) - 2:
                layers.append(nn.ReLU())
        self.net = nn.Sequential(*layers)
        self.device = dev
        self.nb_steps = nb_steps

    def forward(self, x, h):
        x0 = torch.zeros_like(x)
        out = self.net(h)
        offset, scaling = out[:, [0]], torch.exp(out[:, [1]])
        integral = ParallelNeuralIntegral.apply(x0, x, self.integrand, _flatten(self.integrand.parameters()), h,
                                                self.nb_steps)
        return scaling * integral + offset

    def inverse(self, y, h, x_range=(-50., 50.), tol=1e-6, max_iter=64, return_info=False):
        """x [B,1] in ``x_range`` with ``forward(x, h) = y``: y is strictly increasing in x, so x is unique.  The residual is
        driven to ``tol * max(1, |t|)`` on t = (y - o(h)) exp(-s(h)), the value the integral has to reach; a y outside the image
        of ``x_range`` returns the nearer endpoint.  Gradients reach y, h, the conditioner and the integrand (implicit-function
        theorem: one backward launch).  ``return_info=True`` -> (x, f(x; h), status): the integrand at the solution
        (dy/dx = exp(s(h)) f) and an int32 word per row, evaluations used in the low 16 bits, above them
        ``umnn_amd.SOLVE_CLAMPED`` (ended on an endpoint), ``SOLVE_CAPPED`` (still running after ``max_iter``) and ``SOLVE_NONFINITE``."""
        out = self.net(h)
        t = (y - out[:, [0]]) * torch.exp(-out[:, [1]])
        return InverseNeuralIntegral.apply(t, self.integrand, _flatten(self.integrand.parameters()), h, self.nb_steps,
                                           x_range, tol, max_iter, return_info)
