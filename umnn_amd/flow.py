"""UMNN-MAF flow modules: EmbeddingNetwork, UMNNMAF (one block) and UMNNMAFFlow (the stack).

The nn.Module API (constructor arguments, method names, ``.to`` returning self, state_dict keys
``Flow{i}.net.made.net.*``, ``Flow{i}.net.parallel_nets.net.*``, ``Flow{i}.{scaling,pi,cc_weights,cc_steps}``, ``pi``)
is the reference's: models/UMNN/UMNNMAF.py:37-232,304-329 and models/UMNN/UMNNMAFFlow.py:8-151.

What is different underneath (MI355X-first, results unchanged):
  * one block = ONE conditioner pass + ONE fused HIP launch giving both z and log|dz/dx| (quadrature node 0 is x,
    so f(x;h) falls out of the integral; the reference runs MADE twice and the integrand once more,
    UMNNMAFFlow.py:113-114 / UMNNMAF.py:136-139);
  * the node axis is never materialised, so "CC" and "CCParallel" are the same kernel;
  * training goes through ``IntegralWithJacobian`` (HIP forward + HIP backward with the reference's gradient
    convention); inference through the fully fused block epilogue.
Names the reference's scripts call but the reference never defines exist here as aliases.
"""
import math
import os

import numpy as np
import torch
import torch.nn as nn

from . import integral as _I
from . import inverse as _inv
from . import sampling as _S
from .integral import NeuralIntegral, ParallelNeuralIntegral, IntegralWithJacobian, IntegralWithJacobianParams, _flatten  # noqa: F401
from .made import MADE, ConditionnalMADE
from .nets import ELUPlus, IntegrandNetwork, compute_lipschitz_linear, mlp_spec  # noqa: F401  (re-exported)
from .quadrature import compute_cc_weights

_SOLVERS = _I.SOLVERS


class EmbeddingNetwork(nn.Module):
    """Conditioner (MADE) + the shared integrand MLP of one block."""

    def __init__(self, in_d, hiddens_embedding=[50, 50, 50, 50], hiddens_integrand=[50, 50, 50, 50], out_made=1,
                 cond_in=0, act_func='ELU', device="cpu"):
        super().__init__()
        self.m_embeding = None
        self.embedding_dtype = None     # None: whatever the conditioner computes in; torch.bfloat16: configuration C4
        self.device = device
        self.in_d = in_d
        if cond_in > 0:
            self.made = ConditionnalMADE(in_d, cond_in, hiddens_embedding, (in_d + cond_in) * out_made, num_masks=1,
                                         natural_ordering=True).to(device)
        else:
            self.made = MADE(in_d, hiddens_embedding, in_d * out_made, num_masks=1, natural_ordering=True).to(device)
        self.parallel_nets = IntegrandNetwork(in_d, 1 + out_made, hiddens_integrand, 1, act_func=act_func,
                                              device=device)

    def to(self, device):
        self.device = device
        self.made.to(device)
        self.parallel_nets.to(device)
        return self

    def make_embeding(self, x_made, context=None):
        # .raw(): the masked MLP itself.  (The reference calls MADE.forward, whose nout==2 "Gaussian" branch
        # breaks the d=2/E=1 and d=1/E=2 flows, made.py:114-118; the embedding never wants that branch.)
        if isinstance(self.made, ConditionnalMADE):
            self.m_embeding = self.made.raw(x_made, context, out_dtype=self.embedding_dtype)
        else:
            self.m_embeding = self.made.raw(x_made, out_dtype=self.embedding_dtype)
        return self.m_embeding

    def graph_embedding(self, x_made, context, weights):
        """``make_embeding`` for the recorded sampling loops: the conditioner's graph-mode composition on masked weights the caller
        formed once (``made.graph_weights()``); writes no attribute."""
        if isinstance(self.made, ConditionnalMADE):
            return self.made.raw_graph(x_made, context, weights, out_dtype=self.embedding_dtype)
        return self.made.raw_graph(x_made, weights, out_dtype=self.embedding_dtype)

    def forward(self, x_t):
        return self.parallel_nets.forward(x_t, self.m_embeding)


class UMNNMAF(nn.Module):
    def __init__(self, net, input_size, nb_steps=100, device="cpu", solver="CC"):
        super().__init__()
        self.net = net.to(device)
        self.device = device
        self.input_size = input_size
        self.nb_steps = nb_steps
        self.solver = solver
        self.register_buffer("pi", torch.tensor(math.pi))
        # Registered tables keep the CONSTRUCTOR's shape for the whole life of the module, like the reference's
        # (state_dict parity: UCIExperiments.py:131-153 saves after set_steps_nb).  They are checkpoint payload only:
        # the kernels read quadrature.device_tables(self.nb_steps).  nb_steps <= 0 ("0 for random", the scripts then
        # call set_steps_nb per batch) gets NaN placeholders of the reference's shape; n >= 1 is checked when integrating.
        if nb_steps >= 1:
            w, s = compute_cc_weights(nb_steps)
            w, s = w.clone(), s.clone()
        else:
            w = torch.full((max(nb_steps + 1, 0), 1), float("nan"))
            s = w.clone()
        self.register_buffer("cc_weights", w)
        self.register_buffer("cc_steps", s)
        self.scaling = nn.Parameter(torch.zeros(input_size, device=self.device), requires_grad=False)

    def to(self, device):
        self.device = device
        super().to(device)
        return self

    # ------------------------------------------------------------------ core: one pass, both outputs
    def _transform(self, x, context=None, x0=None, want_jac=True, reverse_z=False, log_jac_in=None):
        """-> (z, log_jac or None).  One conditioner pass, one quadrature launch.  ``reverse_z`` / ``log_jac_in`` are
        the glue of a UMNNMAFFlow stack (UMNNMAFFlow.py:109-123): z with its dimensions reversed for the next block,
        log_jac added to the running sum -- inside the kernel on the HIP inference path, with ATen ops otherwise."""
        if self.solver not in _SOLVERS:
            return None, None
        integrand = self.net.parallel_nets
        h = self.net.make_embeding(x, context)
        d = x.shape[1]
        z0 = h.view(h.shape[0], -1, d)[:, 0, :]
        spec = _I._hip_spec(integrand, x)       # (eager and recorded alike; the calls below launch, or record the op of the launch)
        if self.nb_steps < 1:
            raise ValueError("UMNNMAF: nb_steps must be >= 1 when integrating (call set_steps_nb first)")
        # No-graph fast path only when nothing can ask for a gradient.  The reference's eval-mode direct integration
        # (UMNNMAF.py:89-105) stays differentiable through ordinary autograd; here eval + grad-requiring weights /
        # embedding goes through the same autograd Function as training.
        no_graph = (not torch.is_grad_enabled()) or not (
            x.requires_grad or h.requires_grad or (x0 is not None and x0.requires_grad)
            or any(p.requires_grad for p in integrand.parameters()))
        if spec is not None:
            # training: the whole block -- quadrature + epilogue, and their backward -- as ONE autograd node
            one_node = (not no_graph and _I.fused_block_ok(x, h, self.scaling, x0, want_jac)
                        and (log_jac_in is None or log_jac_in.dtype == torch.float32))
            if one_node or (no_graph and x0 is None):
                return _I.flow_block(spec, integrand, x, h, self.scaling, self.nb_steps, reverse_z, log_jac_in, train=one_node)
            x0 = x0.to(x.device) if x0 is not None else None      # None = lower limit 0 inside the kernels
            F, fx = _I.cc_forward_jac(spec, integrand, x0, x, h, self.nb_steps, no_graph)
        else:
            x0 = x0.to(x.device) if x0 is not None else torch.zeros_like(x)
            if no_graph:
                with torch.no_grad():
                    F = _I.aten_forward(integrand, x0, x, h, self.nb_steps)
            else:
                F = _SOLVERS[self.solver].apply(x0, x, integrand, _flatten(integrand.parameters()), h, self.nb_steps)
            fx = integrand(x, h) if want_jac else None
        z = torch.exp(self.scaling).unsqueeze(0) * (F + z0)
        log_jac = torch.log(fx + 1e-10) + self.scaling.unsqueeze(0) if want_jac else None
        if reverse_z:
            z = torch.flip(z, [1])
        if log_jac_in is not None and log_jac is not None:
            log_jac = log_jac_in + log_jac
        return z, log_jac

    # ------------------------------------------------------------------ reference API
    def forward(self, x, method=None, x0=None, context=None):
        return self._transform(x, context, x0, want_jac=False)[0]

    def compute_log_jac(self, x, context=None):
        h = self.net.make_embeding(x, context)
        integrand = self.net.parallel_nets
        spec = _I._hip_spec(integrand, x)
        if spec is not None:
            # f(x;h) is quadrature node 0: a one-step launch of the forward kernel evaluates it (two nodes) without the
            # [B*d, 1+E] row matrix the reference materialises (UMNNMAF.py:136-139, 263-284)
            no_graph = not (torch.is_grad_enabled() and (x.requires_grad or h.requires_grad
                                                         or any(p.requires_grad for p in integrand.parameters())))
            jac = _I.cc_forward_jac(spec, integrand, None, x, h, 1, no_graph)[1]
        else:
            jac = integrand(x, h)
        return torch.log(jac + 1e-10) + self.scaling.unsqueeze(0).expand(x.shape[0], -1)

    def compute_log_jac_bis(self, x, context=None):
        return self._transform(x, context)

    def compute_ll(self, x, context=None):
        z, log_jac = self._transform(x, context)
        z.clamp_(-10., 10.)
        log_prob_gauss = -.5 * (torch.log(self.pi * 2) + z ** 2).sum(1)
        return log_prob_gauss + log_jac.sum(1), z

    def compute_ll_bis(self, x, context=None):
        z, log_jac = self._transform(x, context)
        z.clamp_(-10., 10.)
        return log_jac, z

    def compute_bpp(self, x, alpha=1e-6, context=None):
        d = x.shape[1]
        ll, z = self.compute_ll(x, context=context)
        bpp = -ll / (d * np.log(2)) - np.log2(1 - 2 * alpha) + 8 \
            + 1 / d * (torch.log2(torch.sigmoid(x)) + torch.log2(1 - torch.sigmoid(x))).sum(1)
        z.clamp_(-10., 10.)
        return bpp, ll, z

    def set_steps_nb(self, nb_steps):
        # The registered cc_weights / cc_steps buffers stay at constructor shape (checkpoint round trip, see __init__);
        # every integral reads the tables of the CURRENT nb_steps from the per-device cache, so the reference's
        # stale-buffer crash in eval + CCParallel (UMNNMAF.py:48-50,104-106,172-173) cannot happen here.
        self.nb_steps = nb_steps

    def compute_lipschitz(self, nb_iter=10):
        return self.net.parallel_nets.compute_lipschitz(nb_iter)

    def force_lipschitz(self, L=1.5):
        self.net.parallel_nets.force_lipschitz(L)

    computeLL = compute_ll
    computell = compute_ll
    computeLipshitz = compute_lipschitz
    forceLipshitz = force_lipschitz
    forcei_lpschitz = force_lipschitz

    # ------------------------------------------------------------------ inversion (sampling), row f3: drivers in sampling.py
    def invert(self, z, iter=10, context=None, method="bracket", tol=1e-6, max_iter=64, sweep_tol=1e-6, max_sweeps=None,
               return_info=False, conditioner="full", return_log_jac=False):
        """Dimension-by-dimension bracket search: 10 candidates per round on [left,right] (starting at +-50), keep
        the sub-interval next to the candidate whose image is closest to the target (UMNNMAF.py:182-232).  Under torch.compile /
        torch.export the search is an eager call (a graph break); under torch.jit.trace ``invert`` raises.  On the HIP path
        ``method="newton"`` and ``method="jacobi"`` with ``sweep_tol=0`` and an explicit ``max_sweeps`` ARE recorded
        (``sampling.invert_recorded``: newton unrolls d conditioner + solve steps at trace time -- for small d; wide blocks record jacobi,
        whose ``return_info`` there is {"sweeps": K, "status", "last_move": a 0-dim device tensor}).
        ``method="newton"`` (an extension; ``iter`` is ignored): the same dimension-by-dimension structure with the safeguarded Newton
        solve of ``umnn_cc_solve`` on [-50, 50] in place of the search -- residual to ``tol * max(1, |z_j|)``, at most ``max_iter``
        quadratures per dimension, typically four.
        ``method="jacobi"`` (an extension; ``iter`` is ignored): the Jacobi iteration of ``sampling.invert_jacobi`` -- every sweep is one full
        conditioner pass and ONE solve of all d dimensions under that embedding (``umnn_cc_solve_block``), warm-started from the previous
        sweep; stops when no entry moved by more than ``sweep_tol * max(1, |x|)`` or after ``max_sweeps`` sweeps (default d, where the
        result is the sequential one by construction).  ``return_info=True`` (jacobi only) -> (x, info).
        ``conditioner="progressive"`` (an extension, "newton" and "bracket"; default "full"): the walk keeps every hidden unit of the
        conditioner once it is final (``MADE.progressive_plan``) and per dimension computes only the units that became ready and the E
        outputs of that dimension -- on the HIP path ONE ``umnn_made_step`` launch, so a dimension is two launches; host tensors and
        nets that kernel refuses run the same walk in torch ops.  Conditioners it does not apply to (random input order, several masks,
        other weight dtypes, a bf16 embedding) run "full", announced once.  An eager call under torch.compile / torch.export.
        ``return_log_jac=True`` (an extension) -> (x, log_jac), or (x, info, log_jac) with ``return_info``: log_jac [B] = sum_i
        [log(f(x_i; h_i) + 1e-10) + s_i], the row sum of ``compute_log_jac`` at the returned x, taken from the solves that produced x --
        the last quadrature of a Newton solve has x as its node 0, so f(x) is already there.  "newton" (both conditioners) adds it in the
        solve kernel's epilogue (``umnn_cc_solve_lj``: no launch more), "jacobi" takes the f_x of its sweeps (the same launch) and sums
        it with one ``umnn_flow_sample_lj_rows`` launch per block; host tensors and other dtypes form the same sum in torch ops from
        what ``integral.newton_solve`` returns.  "bracket" is the one method that pays a pass: the search never evaluates f(x), so it
        runs one forward launch of the integrand on its result (``sampling.invert_bracket``: a one-step quadrature, whose node 0 is x, under the
        embedding the search's last dimension left -- no conditioner pass).  x is what the same call returns without the flag, bit for bit.  Not
        differentiable (``invert`` runs under no_grad); gradients of a density go through ``log_prob(x)``."""
        return _S.invert([self], False, "UMNNMAF", z, context, _S.Options(method, iter, tol, max_iter, sweep_tol, max_sweeps, conditioner,
                                                                          bool(return_info), bool(return_log_jac)))

    def inverse(self, z, context=None, method="newton", tol=1e-6, max_iter=64, sweep_tol=1e-6, max_sweeps=None, adj_tol=1e-6,
                max_adj_sweeps=None, return_info=False):
        """x with ``self(x) = z``, DIFFERENTIABLE in z, the block's parameters and the context (``invert`` runs under no_grad): the
        solve of ``invert(method="newton" | "jacobi")`` -- ``tol``, ``max_iter``, ``sweep_tol``, ``max_sweeps`` are its arguments;
        ``"bracket"`` is refused -- as one autograd node, ``inverse.FlowBlockInverse``, whose backward is the implicit gradient: J^T lam =
        g_x by adjoint Jacobi sweeps (one block VJP without parameter gradients and one elementwise launch each), then g_z = lam and one
        more VJP with -lam for the parameters and the context.  The sweeps stop when every |g_x - J^T lam| <= ``adj_tol`` max(1, |g_x|)
        (one 4-byte device-to-host read per sweep; ``adj_tol`` = 0: no test, no read) and in any case after ``max_adj_sweeps`` (default d,
        where lam is exact: J is triangular).  ``return_info=True`` -> (x, info): info["solve"] holds the Jacobi solve's info per block
        (None for newton), info["adjoint"] is filled by the backward with {"sweeps", "vjps", "flags"} per block ("sweeps": the updates
        lam needed -- the first k whose lam^k met the test, or the cap; "vjps": the block VJPs run, one more when the test ended the
        loop; "flags": the last flag word read -- bit 0 not converged, bit 1 a non-finite residual -- or None with ``adj_tol`` = 0).
        In float32 the VJP's own rounding (a few 1e-6 of max(1, |g_x|) once the dimensions are strongly coupled) can sit above the default
        ``adj_tol``: the sweeps then run to the cap -- the exact answer, at d block backwards; ``adj_tol=1e-5`` stops such blocks after
        the 5-7 sweeps the iteration needs (EXPERIMENTS.md).
        The Jacobian is this package's own (dF/dx = f(x), the Leibniz term), so a finite difference of ``invert`` differs by the
        quadrature error of f.  Entries whose solve ended SOLVE_CLAMPED or SOLVE_NONFINITE are not solutions of T(x) = z and have no
        defined gradient; the rows of a batch are independent, so every other sample is unaffected.  Eager only, like ``invert``."""
        return _inv.inverse([self], False, "UMNNMAF.inverse", z, context, method, tol, max_iter, sweep_tol, max_sweeps, adj_tol,
                            max_adj_sweeps, return_info)

    def sample_and_log_prob(self, n, context=None, generator=None, **solve_opts):
        """``UMNNMAFFlow.sample_and_log_prob`` for a single block -> (x [n, d], log_prob [n]); method "newton" by default, under no_grad.
        (The Gaussian term uses the drawn noise itself; ``compute_ll`` of a single block clamps its z to +-10 first.)"""
        return _S.sample_and_log_prob(self, self, n, context, generator, solve_opts)


class ListModule(object):
    """Registers modules on ``module`` as attributes ``prefix0, prefix1, ...`` and indexes them like a list."""

    def __init__(self, module, prefix, *args):
        self.module, self.prefix, self.num_module = module, prefix, 0
        for m in args:
            self.append(m)

    def append(self, new_module):
        if not isinstance(new_module, nn.Module):
            raise ValueError('Not a Module')
        self.module.add_module(self.prefix + str(self.num_module), new_module)
        self.num_module += 1

    def __len__(self):
        return self.num_module

    def __getitem__(self, i):
        if not 0 <= i < self.num_module:
            raise IndexError('Out of bound')
        return getattr(self.module, self.prefix + str(i))


class UMNNMAFFlow(nn.Module):
    def __init__(self, nb_flow=1, nb_in=1, hidden_derivative=[50, 50, 50, 50], hidden_embedding=[50, 50, 50, 50],
                 embedding_s=20, nb_steps=50, act_func='ELU', solver="CC", cond_in=0, device="cpu"):
        super().__init__()
        self.device = device
        self.register_buffer("pi", torch.tensor(math.pi))
        self.nets = ListModule(self, "Flow")
        for _ in range(nb_flow):
            emb = EmbeddingNetwork(nb_in, hidden_embedding, hidden_derivative, embedding_s, act_func=act_func,
                                   device=device, cond_in=cond_in).to(device)
            self.nets.append(UMNNMAF(emb, nb_in, nb_steps, device, solver=solver).to(device))

    def to(self, device):
        for net in self.nets:
            net.to(device)
        self.device = device
        super().to(device)
        return self

    def _stack(self, x, context, want_jac):
        """Run the blocks with the dimension reversal between them -> (z in original order, summed log_jac)."""
        log_jac = None
        nb = len(self.nets)
        for i, net in enumerate(self.nets):
            # every block but the last hands its z over reversed (the reference flips after every block and once more
            # at the end: the last two flips cancel); log_jac accumulates elementwise in each block's own input order
            x, lj = net._transform(x, context, want_jac=want_jac, reverse_z=i + 1 < nb, log_jac_in=log_jac)
            if want_jac:
                log_jac = lj
        return x, (log_jac if want_jac else 0.)

    def forward(self, x, context=None):
        return self._stack(x, context, False)[0]

    def invert(self, z, iter=10, context=None, method="bracket", tol=1e-6, max_iter=64, sweep_tol=1e-6, max_sweeps=None,
               return_info=False, conditioner="full", return_log_jac=False):
        """Sampling direction, block by block.  ``method="bracket"`` (default): the reference's search, ``iter`` rounds.
        ``method="newton"``: the in-kernel Newton solve (``UMNNMAF.invert``), exactly nb_flow x d solve launches; ``iter`` is ignored.
        ``method="jacobi"``: the Jacobi iteration of ``UMNNMAF.invert`` in every block, one solve launch per sweep;
        ``return_info=True`` -> (x, info) with info's entries as lists over the blocks in flow order.
        torch.compile / torch.export record "newton" and fixed-sweep "jacobi" (``sweep_tol=0``, ``max_sweeps=K``) on the HIP path, see
        ``UMNNMAF.invert``; everything else stays an eager call there.  ``conditioner``: see ``UMNNMAF.invert``.
        ``return_log_jac=True`` -> (x, log_jac), or (x, info, log_jac) with ``return_info``: log_jac [B] = the sum over the blocks of
        ``UMNNMAF.invert``'s, i.e. ``compute_log_jac(x).sum(1)`` at the returned x from the solves that produced it -- one running sum
        the solve launches of every block add to ("newton"), one ``umnn_flow_sample_lj_rows`` launch per block ("jacobi"), one block
        forward per block ("bracket", the one method that pays a pass).  x is bit-identical to the call without the flag.  Not
        differentiable: ``inverse`` / ``rsample`` are untouched, and their users call ``log_prob(x)``."""
        blocks = [self.nets[i] for i in range(len(self.nets))]
        return _S.invert(blocks, True, "UMNNMAFFlow", z, context, _S.Options(method, iter, tol, max_iter, sweep_tol, max_sweeps, conditioner,
                                                                             bool(return_info), bool(return_log_jac)))

    def inverse(self, z, context=None, method="newton", tol=1e-6, max_iter=64, sweep_tol=1e-6, max_sweeps=None, adj_tol=1e-6,
                max_adj_sweeps=None, return_info=False):
        """The sampling direction with gradients to z, every parameter and the context: ``UMNNMAF.inverse`` block by block, walking
        the blocks and flipping as ``invert(method="newton")`` does (the flips are ordinary differentiable ops).  ``return_info=True``
        -> (x, info) with info["solve"] / info["adjoint"] as lists over the blocks in flow order; the backward fills info["adjoint"]."""
        return _inv.inverse(self.nets, True, "UMNNMAFFlow.inverse", z, context, method, tol, max_iter, sweep_tol, max_sweeps, adj_tol,
                            max_adj_sweeps, return_info)

    def sample(self, n, context=None, generator=None, **solve_opts):
        """n samples x = T^-1(z), z ~ N(0, I), without a graph: ``invert`` (method "newton" unless ``solve_opts`` says otherwise).
        Recorded by torch.compile / torch.export where ``invert`` is, when no generator is given."""
        solve_opts.setdefault("method", "newton")
        with torch.no_grad():
            return self.invert(_S.base_noise(self.pi, self.nets[0], n, generator), context=context, **solve_opts)

    def rsample(self, n, context=None, generator=None, **opts):
        """n reparameterised samples: ``inverse`` of z ~ N(0, I), differentiable in the parameters and the context."""
        return self.inverse(_S.base_noise(self.pi, self.nets[0], n, generator), context=context, **opts)

    def sample_and_log_prob(self, n, context=None, generator=None, **solve_opts):
        """n samples with their log-density -> (x [n, d], log_prob [n]): ``sample`` whose solves also hand over f(x), the diagonal of
        every block's Jacobian (``invert(..., return_log_jac=True)``), so that
            log q(x) = sum_blocks sum_i [log(f(x_i) + 1e-10) + s_i] - 1/2 sum_i (log 2 pi + z_i^2),   z the noise x was drawn from,
        ``compute_ll``'s formula term by term, costs no second conditioner and quadrature pass (``sample`` + ``log_prob(x)`` runs
        both again); the Gaussian term is one ``umnn_flow_sample_ll`` launch, or the same arithmetic in torch ops off the HIP path
        and in recorded graphs.  x is the x of ``sample`` with the same generator state and options.  It differs from ``log_prob(x)``
        by the solve's residual only (z against T(x): at most ``tol`` max(1, |z|) per dimension).  Runs under no_grad: a density to
        differentiate is ``log_prob(x)``, and reparameterised samples come from ``rsample``."""
        return _S.sample_and_log_prob(self, self.nets[0], n, context, generator, solve_opts)

    def log_prob(self, x, context=None):
        return self.compute_ll(x, context)[0]

    def compute_log_jac(self, x, context=None):
        return self._stack(x, context, True)[1]

    def compute_log_jac_bis(self, x, context=None):
        return self._stack(x, context, True)

    def _one_pass_specs(self, x):
        """The integrand specs of the blocks when the fused one-pass log-likelihood (umnn_flow_ll_block_forward) applies, else None:
        HIP path, fp32, nothing can ask for a gradient (same rule as UMNNMAF._transform)."""
        if len(self.nets) == 0 or not x.is_cuda or x.dtype != torch.float32 or x.dim() != 2 or torch.is_autocast_enabled():
            return None
        specs, graph = [], _I._graph_mode()
        for net in self.nets:
            # (the one-pass entry point is fp32-only; bf16 storage takes the _io route)
            if net.solver not in _SOLVERS or net.nb_steps < 1 or net.net.embedding_dtype not in (None, torch.float32):
                return None
            specs.append(_I._hip_spec(net.net.parallel_nets, x, graph))
            if specs[-1] is None:
                return None
        if torch.is_grad_enabled() and (x.requires_grad or any(p.requires_grad for p in self.parameters())):
            return None
        return specs

    def compute_ll(self, x, context=None):
        specs = self._one_pass_specs(x)
        if specs is not None:
            # nb_flow x (conditioner + ONE launch): z, the running per-sample log-likelihood and the Gaussian term all
            # leave the quadrature kernel; no [B,d] log_jac accumulation, no elementwise epilogue (UMNNMAFFlow.py:109-119)
            with torch.no_grad():
                x = x.contiguous()
                work, ll, nb = _I.flow_ll_workspace(x), None, len(self.nets)
                for i, (net, spec) in enumerate(zip(self.nets, specs)):
                    h = net.net.make_embeding(x, context)
                    x, ll = _I.flow_ll_link(spec, x, h.contiguous(), net.scaling, net.nb_steps, i + 1 < nb, i == 0, i + 1 == nb, ll, work)
            return ll, x
        z, log_jac = self._stack(x, context, True)
        if (z.is_cuda and z.dtype == torch.float32 and log_jac.dtype == torch.float32 and z.dim() == 2 and torch.is_grad_enabled()
                and (z.requires_grad or log_jac.requires_grad) and not torch.is_autocast_enabled()
                and os.environ.get("UMNN_FUSED_TRAIN", "1") != "0"):
            return _I.flow_ll(z, log_jac), z        # (training: the reduction and its backward as one launch each)
        log_prob_gauss = -.5 * (torch.log(self.pi * 2) + z ** 2).sum(1)
        return log_jac.sum(1) + log_prob_gauss, z

    def compute_ll_bis(self, x, context=None):
        z, log_jac = self._stack(x, context, True)
        return log_jac + -.5 * (torch.log(self.pi * 2) + z ** 2), z

    def compute_bpp(self, x, alpha=1e-6, context=None):
        d = x.shape[1]
        ll, z = self.compute_ll(x, context=context)
        bpp = -ll / (d * np.log(2)) - np.log2(1 - 2 * alpha) + 8 \
            + 1 / d * (torch.log2(torch.sigmoid(x)) + torch.log2(1 - torch.sigmoid(x))).sum(1)
        return bpp, ll, z

    def set_steps_nb(self, nb_steps):
        for net in self.nets:
            net.set_steps_nb(nb_steps)

    def set_embedding_dtype(self, dtype):
        """Storage type of the [B, E*d] embedding h between the conditioner and the quadrature kernels (an extension of
        this package, configuration C4): ``torch.bfloat16`` makes the conditioner's last GEMM write bf16 and the kernels
        read it with bf16 loads (fp32 arithmetic inside); ``None`` restores the conditioner's own dtype."""
        for net in self.nets:
            net.net.embedding_dtype = dtype

    def compute_lipschitz(self, nb_iter=10):
        L = 1.
        for net in self.nets:
            L *= net.compute_lipschitz(nb_iter)
        return L

    def force_lipschitz(self, L=1.5):
        for net in self.nets:
            net.force_lipschitz(L)

    computell = compute_ll
    computeLL = compute_ll
    computeLipshitz = compute_lipschitz
    forceLipshitz = force_lipschitz
    forcei_lpschitz = force_lipschitz
