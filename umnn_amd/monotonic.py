"""MonotonicNN: a scalar function monotone in x, y = exp(s(h)) * int_0^x f(t;h) dt + o(h).

Mirrors models/UMNN/MonotonicNN.py:29-54 (constructor ``MonotonicNN(in_d, hidden_layers, nb_steps=50, dev="cpu")``,
``forward(x, h)`` with x [B,1] and h [B,in_d-1], state_dict keys ``integrand.net.*`` / ``net.*``).  The integral is
the same HIP kernel as the flow's (d = 1, E = in_d-1, ReLU hidden layers).

``n_out=K`` (an extension of this package, last in the signature: the reference's positional arguments and, at ``n_out=1``, its
state_dict shapes and results are untouched) makes it K monotone functions of the same x under the same covariates -- a CDF per
class, one curve per risk -- that share every hidden layer of the integrand: ``forward`` returns [B, K], y_k = exp(s_k(h)) *
int_0^x f_k(t;h) dt + o_k(h), the conditioner ending in 2K units (offsets first, log-scales after).  On GPU tensors the K
integrals are ONE launch of the multi-output kernels (csrc/cc_multi.hip: exact fp32, whatever ``set_precision`` says).

``inverse(y, h)`` (an extension of this package: the reference has no such method) returns the x with forward(x, h) = y --
quantile functions, inverse-CDF sampling, calibration maps -- by the in-kernel Newton solve, differentiable in y, h and every parameter;
``output=k`` picks the function to invert when ``n_out > 1``.  ``inverse_sum(y, h, weights)`` inverts a non-negative combination
sum_k w_k y_k of the K curves -- the event time of competing risks, a quantile of a mixture of CDFs -- in one solve launch.

``forward_curve(x, h)`` returns the whole curve t -> forward(t, h) at the nb_steps + 1 quadrature nodes of [0, x] for the work of ONE
``forward`` (the kernel keeps the node values it used to sum away; csrc/cc_cumulate.hip integrates them up to every node), and
``cumulative_incidence(x, h)`` the nested integral CIF_k(t) = int_0^t y_k'(s) exp(-sum_j y_j(s)) ds from the same nodes.
"""
import torch
import torch.nn as nn
import torch.nn.functional as F

from .integral import IntegralCurve, IntegralWithDerivative, InverseIntegralSum, cumulate, InverseNeuralIntegral, ParallelNeuralIntegral, _flatten
from .nets import IntegrandNN, MlpSpec, TensorLinear, _spec_from_sequential  # noqa: F401  (IntegrandNN is re-exported)


class OutputRow(nn.Module):
    """Output k of a multi-output ``IntegrandNN`` as a single-output integrand: a VIEW -- the hidden layers themselves and row k of
    the last layer (``W_L[k:k+1]``, ``b_L[k:k+1]``) -- so the existing single-output solve and backward kernels run on it unchanged.
    It owns no parameters: ``row_params()`` are the tensors a gradient flows back through (into row k only), in the order of the flat
    d_theta of its spec."""

    def __init__(self, integrand, k):
        super().__init__()
        object.__setattr__(self, "base", integrand)           # (not a submodule: parameters() stays empty)
        self.k = int(k)

    def _linears(self):
        return [m for m in self.base.net if isinstance(m, nn.Linear)]

    def row_params(self):
        lins, k = self._linears(), self.k
        out = [p for lin in lins[:-1] for p in (lin.weight, lin.bias)]
        return out + [lins[-1].weight[k:k + 1], lins[-1].bias[k:k + 1]]

    @staticmethod
    def _mlp(params, x, h):
        a = torch.cat((x, h), 1)
        n = len(params) // 2
        for l in range(n):
            a = F.linear(a, params[2 * l], params[2 * l + 1])
            if l + 1 < n:
                a = F.relu(a)
        return F.elu(a) + 1.

    def forward(self, x, h):
        return self._mlp(self.row_params(), x, h)

    def _umnn_pure(self):
        return (lambda ps, t, h: self._mlp(ps, t, h)), [p.detach() for p in self.row_params()]

    def _umnn_spec(self):
        spec = _spec_from_sequential(self.base.net, plus_one_outside=True)
        if spec is None:
            return None
        last, k = spec.linears[-1], self.k
        return MlpSpec(spec.linears[:-1] + [TensorLinear(last.weight[k:k + 1], last.bias[k:k + 1])], spec.hidden_act, spec.out_act)


class MonotonicNN(nn.Module):
    def __init__(self, in_d, hidden_layers, nb_steps=50, dev="cpu", n_out=1):
        super().__init__()
        self.n_out = int(n_out)
        self.integrand = IntegrandNN(in_d, hidden_layers, self.n_out)
        sizes = [in_d - 1] + list(hidden_layers) + [2 * self.n_out]      # conditioner -> (offsets, log-scales)
        layers = []
        for i in range(len(sizes) - 1):
            layers.append(nn.Linear(sizes[i], sizes[i + 1]))
            if i < len(sizes) - 2:
                layers.append(nn.ReLU())
        self.net = nn.Sequential(*layers)
        self.device = dev
        self.nb_steps = nb_steps

    def _offset_log_scaling(self, h, k=None):
        """The conditioner's output, split -> (o(h), s(h)): every output ([B, n_out] each), or output ``k`` alone ([B, 1] each).
        ``n_out == 1`` is its output 0 in the indexing form of the reference (MonotonicNN.py:47-48), which decides the autograd nodes."""
        out = self.net(h)
        if k is None and self.n_out == 1:
            k = 0
        if k is not None:
            return out[:, [k]], out[:, [self.n_out + k]]
        return out[:, :self.n_out], out[:, self.n_out:]

    def forward(self, x, h):
        x0 = torch.zeros_like(x)
        offset, log_scaling = self._offset_log_scaling(h)
        scaling = torch.exp(log_scaling)
        integral = ParallelNeuralIntegral.apply(x0, x, self.integrand, _flatten(self.integrand.parameters()), h,
                                                self.nb_steps)
        return scaling * integral + offset

    def forward_with_derivative(self, x, h, log=False):
        """(y [B, n_out], dy/dx [B, n_out]): ``forward(x, h)`` and its derivative in x, dy_k/dx = exp(s_k(h)) f_k(x; h) > 0 -- the
        density of a CDF, the hazard of a cumulative hazard, the Jacobian of a change of variables.  ``log=True`` returns
        log dy_k/dx = s_k(h) + log f_k(x; h) instead, what a likelihood consumes (no overflow through exp).  f_k(x; h) is node 0 of the
        quadrature, so on GPU tensors the pair is ONE quadrature launch for every ``n_out`` (``IntegralWithDerivative``), and
        gradients of both outputs reach x, h, the conditioner and the integrand through the backward kernels.

        This is the package's replacement for ``torch.autograd.grad(y, x, create_graph=True)``: the quadrature operators are
        once-differentiable by design, so that call keeps raising; a double backward through this pair is out of scope too."""
        x0 = torch.zeros_like(x)
        offset, log_scaling = self._offset_log_scaling(h)
        scaling = torch.exp(log_scaling)
        integral, f_x = IntegralWithDerivative.apply(x0, x, self.integrand, _flatten(self.integrand.parameters()), h, self.nb_steps)
        return scaling * integral + offset, (log_scaling + torch.log(f_x) if log else scaling * f_x)

    def inverse(self, y, h, x_range=(-50., 50.), tol=1e-6, max_iter=64, return_info=False, output=0):
        """x [B,1] in ``x_range`` with ``forward(x, h) = y`` (``forward(x, h)[:, output] = y`` when ``n_out > 1``): y is strictly
        increasing in x, so x is unique.  The residual is
        driven to ``tol * max(1, |t|)`` on t = (y - o(h)) exp(-s(h)), the value the integral has to reach; a y outside the image
        of ``x_range`` returns the nearer endpoint.  Gradients reach y, h, the conditioner and the integrand (implicit-function
        theorem: one backward launch; with ``n_out > 1`` the solve and its backward are the single-output kernels on row ``output`` of
        the integrand's last layer, whose other rows get zero gradient).  ``return_info=True`` -> (x, f(x; h), status): the integrand at the solution
        (dy/dx = exp(s(h)) f) and an int32 word per row, evaluations used in the low 16 bits, above them
        ``umnn_amd.SOLVE_CLAMPED`` (ended on an endpoint), ``SOLVE_CAPPED`` (still running after ``max_iter``) and ``SOLVE_NONFINITE``."""
        k = int(output)
        if not 0 <= k < self.n_out:
            raise IndexError(f"MonotonicNN.inverse: output {output} of a model with n_out = {self.n_out}")
        offset, log_scaling = self._offset_log_scaling(h, k)
        t = (y - offset) * torch.exp(-log_scaling)
        if self.n_out == 1:
            return InverseNeuralIntegral.apply(t, self.integrand, _flatten(self.integrand.parameters()), h, self.nb_steps,
                                               x_range, tol, max_iter, return_info)
        row = OutputRow(self.integrand, k)
        return InverseNeuralIntegral.apply(t, row, _flatten(row.row_params()), h, self.nb_steps, x_range, tol, max_iter, return_info)

    def inverse_sum(self, y, h, weights=None, x_range=(-50., 50.), tol=1e-6, max_iter=64, return_info=False):
        """x [B,1] in ``x_range`` with ``sum_k w_k forward(x, h)[:, k] = y``: the inverse of a non-negative combination of the
        ``n_out`` curves, which is increasing in x like each of them -- the event time T of competing risks, sum_k H_k(T) = -log U
        (median survival at y = log 2), a quantile of the mixture sum_k pi_k F_k.  ``weights``: None (all ones), [n_out], or
        [B, n_out] (which may come from a network and receives gradients); they must be non-negative with a positive one per row
        -- documented, not checked: a check would synchronise -- and a row of zeros follows the clamping rule.  On GPU tensors the
        solve is ONE launch (``InverseIntegralSum``: the Newton iteration runs inside the K-output quadrature kernel) on
        coef = w exp(s(h)) and t = y - sum_k w_k o_k(h), to ``tol * max(1, |t|)``.  Gradients reach y, the weights, h, the
        conditioner and the integrand.  ``return_info=True`` -> (x, f_k(x; h) [B, n_out], status): cause k then has probability
        proportional to coef_k f_k; status as in ``inverse``.  ``n_out == 1`` is ``inverse`` of y / w."""
        offset, log_scaling = self._offset_log_scaling(h)
        w = torch.ones_like(offset) if weights is None else weights.to(offset.dtype).expand_as(offset)
        coef = w * torch.exp(log_scaling)
        t = y - (w * offset).sum(1, keepdim=True)
        if self.n_out == 1:
            return InverseNeuralIntegral.apply(t / coef, self.integrand, _flatten(self.integrand.parameters()), h, self.nb_steps,
                                               x_range, tol, max_iter, return_info)
        return InverseIntegralSum.apply(t, coef, self.integrand, _flatten(self.integrand.parameters()), h, self.nb_steps,
                                        x_range, tol, max_iter, return_info)

    def forward_curve(self, x, h, with_derivative=False, backward="aten"):
        """(t [B, n+1], y [B, n+1, n_out]) with n = nb_steps: ``forward(t, h)`` on the whole grid t[b] of the n + 1 quadrature nodes
        of [0, x_b], ascending -- t[:, 0] = 0, t[:, n] = x, y[:, n] = ``forward(x, h)`` up to rounding --, for the integrand
        evaluations of ONE ``forward``: a survival curve on a time grid, a CDF to plot or calibrate.  y[:, i, k] = exp(s_k(h)) *
        int_0^{t_i} f_k + o_k(h).  ``with_derivative=True`` -> (t, y, dy/dt [B, n+1, n_out]), dy_k/dt = exp(s_k(h)) f_k(t; h).  Rows
        that share x share their abscissae: a common grid for a batch is x = t_max for every row (descending t for x < 0).  The
        curve points are as accurate as separate nb_steps-node quadratures to each t_i; values between the nodes are not provided.
        On GPU tensors under ``torch.no_grad()`` (or when nothing requires grad) this is two launches (``IntegralCurve``); when a
        gradient can be asked for it runs on ATen under plain autograd, differentiable in x, h and every parameter -- or, with
        ``backward="hip"``, on the same two launches with a backward on the kernels (one adjoint-cumulate launch and the passes of
        the multi-output backward with a cotangent per node; what they do not take falls back to ATen with a notice, never an
        error).  Either way the gradient is the exact one of the DISCRETISED curve: every node t_i = x u_i / 2 moves with x, so
        d y[:, i] / dx is not f at a single point -- deliberately not the Leibniz convention dF/dx = f(x) of ``forward``."""
        offset, log_scaling = self._offset_log_scaling(h)
        scaling = torch.exp(log_scaling).unsqueeze(1)
        # (d_theta of the HIP backward arrives through flat_params; nothing else reads it, so no other call builds it)
        flat = _flatten(self.integrand.parameters()) if backward == "hip" and torch.is_grad_enabled() else None
        t, C, f = IntegralCurve.apply(None, x, self.integrand, flat, h, self.nb_steps, backward)
        y = scaling * C + offset.unsqueeze(1)
        return (t, y, scaling * f) if with_derivative else (t, y)

    def cumulative_incidence(self, x, h, curve=False, backward="aten"):
        """The cumulative incidence of each of the ``n_out`` competing risks whose cumulative hazards are the outputs,
        CIF_k(x) = int_0^x hz_k(s) exp(-sum_j H_j(s)) ds with H = ``forward_curve``'s y and hz = its dy/dt, -> [B, n_out]; ``curve=True``
        -> (t [B, n+1], CIF [B, n+1, n_out]) on ``forward_curve``'s grid, whose last row is that end point.  The inner integrals at
        the nodes of the outer one are the curve itself, so the nested integral costs one more cumulative-quadrature launch on
        top of ``forward_curve`` (three launches on GPU tensors) instead of a quadrature per node.  Gradients as in ``forward_curve``;
        ``backward="hip"`` keeps the third launch under autograd too (its backward is one more adjoint-cumulate launch)."""
        t, H, hz = self.forward_curve(x, h, with_derivative=True, backward=backward)
        cif = cumulate(hz * torch.exp(-H.sum(2, keepdim=True)), None, x, self.nb_steps, backward)
        return (t, cif) if curve else cif[:, -1]
