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
from .integral import NeuralIntegral, ParallelNeuralIntegral, IntegralWithJacobian, IntegralWithJacobianParams, _flatten  # noqa: F401
from .made import MADE, ConditionnalMADE
from .nets import ELUPlus, IntegrandNetwork, compute_lipschitz_linear, mlp_spec  # noqa: F401  (re-exported)
from .quadrature import compute_cc_weights

_SOLVERS = {"CC": NeuralIntegral, "CCParallel": ParallelNeuralIntegral}


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


def _recorded_blocks(cls, flow, z, method, sweep_tol, max_sweeps):
    """The blocks of ``flow`` when this ``invert`` call, met while torch.compile / torch.export trace, is one the graph can hold:
    "newton", or "jacobi" with a fixed sweep count (``sweep_tol`` = 0 and ``max_sweeps`` given: no host read decides anything), fp32
    z and every block on the HIP path (``integral._hip_spec``).  None otherwise: the caller then makes today's eager call."""
    if method == "bracket" or (method == "jacobi" and (sweep_tol != 0 or max_sweeps is None)):
        return None
    blocks = [flow] if cls is UMNNMAF else [flow.nets[i] for i in range(len(flow.nets))]
    if len(blocks) == 0 or z.dim() != 2 or z.dtype != torch.float32:
        return None
    for blk in blocks:
        if blk.solver not in _SOLVERS or blk.nb_steps < 1 or _I._hip_spec(blk.net.parallel_nets, z, True) is None:
            return None
    return blocks


def _invert_recorded(cls, blocks, z, context, method, tol, max_iter, max_sweeps, return_info, return_log_jac=False):
    """``invert`` as torch.compile / torch.export record it: the block walk of ``_invert_newton`` / ``_invert_jacobi`` on
    ``UMNNMAF._invert_block_recorded``.  info (jacobi): "sweeps" = K, the last sweep's "status" and "last_move" = max |x_K - x_{K-1}| /
    max(1, |x_K|), a 0-dim device tensor the caller may test afterwards (NaN when a row ended non-finite) -- per block, as lists
    over the blocks in flow order for a UMNNMAFFlow.  ``return_log_jac``: the blocks' row sums of log(f_x + 1e-10) + s, composed in torch
    ops from the f_x the solve ops return, are appended to the result."""
    stack = cls is not UMNNMAF
    K = None if method == "newton" else int(max_sweeps)
    if K is not None and K < 1:
        raise ValueError("umnn_amd: invert(method='jacobi') needs max_sweeps >= 1")
    status, moves, lj = [], [], None
    with torch.no_grad():
        if stack:
            z = torch.flip(z, [1])
        for blk in reversed(blocks):
            z, st, mv, lj_blk = blk._invert_block_recorded(torch.flip(z, [1]) if stack else z, context, tol, max_iter, K, return_log_jac)
            status.insert(0, st)
            moves.insert(0, mv)
            if return_log_jac:
                lj = lj_blk if lj is None else lj + lj_blk
    out = (z,)
    if return_info:
        out += ({"sweeps": [K] * len(blocks), "status": status, "last_move": moves} if stack
                else {"sweeps": K, "status": status[0], "last_move": moves[0]},)
    if return_log_jac:
        out += (lj,)
    return out[0] if len(out) == 1 else out


def _invert_dispatch(cls, flow, z, iter, context, method, tol, max_iter, sweep_tol, max_sweeps, return_info, conditioner="full",
                     return_log_jac=False):
    """``cls.invert`` of UMNNMAF and UMNNMAFFlow: checks the options and runs ``cls._invert`` / ``_invert_newton`` / ``_invert_jacobi``.
    While torch.compile / torch.export trace, "newton" and fixed-sweep "jacobi" on the HIP path are recorded (``_invert_recorded``);
    every other call there is an eager call the graph breaks at, and torch.jit.trace raises.  ``return_log_jac``: the internal walks
    also return the summed log-Jacobian [B] of the forward map at the x they return; it comes last in the result."""
    if method not in ("bracket", "newton", "jacobi"):
        raise ValueError(f"umnn_amd: unknown inversion method {method!r}; expected 'bracket', 'newton' or 'jacobi'")
    if conditioner not in ("full", "progressive"):
        raise ValueError(f"umnn_amd: unknown conditioner {conditioner!r}; expected 'full' or 'progressive'")
    if method == "jacobi" and conditioner != "full":
        raise ValueError("umnn_amd: conditioner='progressive' belongs to the dimension-by-dimension walks (method 'newton' or 'bracket'); "
                         "a Jacobi sweep needs the whole conditioner")
    if torch.jit.is_tracing():
        raise RuntimeError(f"umnn_amd: {cls.__name__}.invert cannot be traced by torch.jit.trace (data-dependent bracket search); "
                           "call it eagerly")
    if return_info and method != "jacobi":
        raise ValueError("umnn_amd: return_info is an option of invert(method='jacobi')")
    if torch.compiler.is_compiling() and conditioner == "full":      # (the progressive walk is an eager call, like "bracket")
        blocks = _recorded_blocks(cls, flow, z, method, sweep_tol, max_sweeps)
        if blocks is not None:
            return _invert_recorded(cls, blocks, z, context, method, tol, max_iter, max_sweeps, return_info, return_log_jac)
    want_lj = bool(return_log_jac)
    if want_lj and z.shape[0] == 0 and not torch.compiler.is_compiling():
        # nothing to solve (the walks' generic loops cannot shape an empty embedding): empty results of the walks' dtypes
        x = torch.zeros_like(z, dtype=torch.float32 if method == "bracket" else z.dtype)
        lj = torch.zeros(0, device=z.device, dtype=flow.pi.dtype if method == "bracket" else z.dtype)
        if not return_info:
            return x, lj
        one = {"sweeps": 0, "converged": True, "status": torch.zeros(z.shape, device=z.device, dtype=torch.int32), "max_evals": []}
        nb = 1 if cls is UMNNMAF else len(flow.nets)
        return x, (one if cls is UMNNMAF else {k: [v] * nb for k, v in one.items()}), lj
    fn, args = {"bracket": (cls._invert, (z, iter, context, conditioner, want_lj)),
                "newton": (cls._invert_newton, (z, context, tol, max_iter, conditioner, want_lj)),
                "jacobi": (cls._invert_jacobi, (z, context, tol, max_iter, sweep_tol, max_sweeps, return_info, None, want_lj))}[method]
    if torch.compiler.is_compiling():
        # (applied here, not as a decorator: torch.compiler.disable imports torch._dynamo, ~1 s at every package import)
        fn = torch.compiler.disable(fn)
    out = fn(flow, *args)
    if method != "jacobi":
        return out
    if not want_lj:
        return out if return_info else out[0]
    return out if return_info else (out[0], out[2])


def _sample_and_log_prob(flow, n, context, generator, solve_opts):
    """``sample_and_log_prob`` of UMNNMAF and UMNNMAFFlow: noise, ``invert(..., return_log_jac=True)``, the Gaussian term."""
    solve_opts.setdefault("method", "newton")
    if solve_opts.pop("return_info", False):
        raise ValueError("umnn_amd: sample_and_log_prob returns (x, log_prob); ask invert(..., return_info=True, return_log_jac=True) for the info")
    with torch.no_grad():
        z = flow._base_noise(n, generator)
        x, lj = flow.invert(z, context=context, return_log_jac=True, **solve_opts)
        return x, _I.sample_ll(z.contiguous(), lj.contiguous(), flow.pi)


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

    # ------------------------------------------------------------------ inversion (sampling), row f3
    def _conditional_integral(self, cand, h_j):
        """int_0^cand f(t; h_j) dt for one dimension: cand [R,1], h_j [R,E] -> [R,1]."""
        integrand = self.net.parallel_nets
        spec = mlp_spec(integrand)
        if _I._use_hip(spec, cand):
            return _I.hip_forward(spec, None, cand, h_j, self.nb_steps)[0]
        with torch.no_grad():
            return _I.aten_forward(lambda t, hh: integrand.independant_forward(torch.cat((t, hh), 1)),
                                   torch.zeros_like(cand), cand, h_j, self.nb_steps)

    def invert(self, z, iter=10, context=None, method="bracket", tol=1e-6, max_iter=64, sweep_tol=1e-6, max_sweeps=None,
               return_info=False, conditioner="full", return_log_jac=False):
        """Dimension-by-dimension bracket search: 10 candidates per round on [left,right] (starting at +-50), keep
        the sub-interval next to the candidate whose image is closest to the target (UMNNMAF.py:182-232).  Under torch.compile /
        torch.export the search is an eager call (a graph break); under torch.jit.trace ``invert`` raises.  On the HIP path
        ``method="newton"`` and ``method="jacobi"`` with ``sweep_tol=0`` and an explicit ``max_sweeps`` ARE recorded
        (``_invert_block_recorded``: newton unrolls d conditioner + solve steps at trace time -- for small d; wide blocks record jacobi,
        whose ``return_info`` there is {"sweeps": K, "status", "last_move": a 0-dim device tensor}).
        ``method="newton"`` (an extension; ``iter`` is ignored): the same dimension-by-dimension structure with the safeguarded Newton
        solve of ``umnn_cc_solve`` on [-50, 50] in place of the search -- residual to ``tol * max(1, |z_j|)``, at most ``max_iter``
        quadratures per dimension, typically four.
        ``method="jacobi"`` (an extension; ``iter`` is ignored): the Jacobi iteration of ``_invert_jacobi`` -- every sweep is one full
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
        runs one forward launch of the integrand on its result (``_invert``: a one-step quadrature, whose node 0 is x, under the
        embedding the search's last dimension left -- no conditioner pass).  x is what the same call returns without the flag, bit for bit.  Not
        differentiable (``invert`` runs under no_grad); gradients of a density go through ``log_prob(x)``."""
        return _invert_dispatch(UMNNMAF, self, z, iter, context, method, tol, max_iter, sweep_tol, max_sweeps, return_info, conditioner,
                                return_log_jac)

    def _dim_embedding(self, x_inv, context, rows_ok, conditioner="full"):
        """The conditioner pass of the dimension-by-dimension sampling loops -> ``embed(j, widen)``: the embedding h [B, E*d] that
        dimension j is solved under, from ``x_inv``'s current contents.  Dimension j reads E of the E*d embedding entries.  Wide
        unconditional conditioners compute only those columns of their last layer (MADE.raw_rows: for d = 784 that layer is 23 520 rows
        of which 30 are read) into a standing buffer, where ``rows_ok`` (the in-kernel path) and the conditioner allow it; otherwise a
        full pass, with ``widen`` as contiguous fp32 -- exact for a bf16 embedding (set_embedding_dtype, autocast), which the fp32-only
        entry points would misread.
        ``conditioner="progressive"``: ``embed(j, widen)`` is one step of ``made.ProgressiveWalk`` into its standing embedding buffer --
        on the HIP path (``rows_ok``, fp32 x_inv on the weights' device) one ``umnn_made_step`` launch, else the same walk in torch ops."""
        made = self.net.made
        B, d = x_inv.shape
        dev = x_inv.device
        E = made.nout // made.nin
        if conditioner == "progressive":
            plan = made.progressive_plan(dev) if self.net.embedding_dtype in (None, torch.float32) and not torch.is_autocast_enabled() else None
            if plan is None:
                _I._warn_once("progressive-ineligible",
                              "umnn_amd: conditioner='progressive' needs a MADE with the natural input order, one mask, fp32 weights on "
                              "the tensors' device and an fp32 embedding; this one runs conditioner='full'.")
            else:
                use_kernel = bool(rows_ok and x_inv.is_cuda and x_inv.dtype == torch.float32 and x_inv.is_contiguous())
                if rows_ok and x_inv.is_cuda and plan.desc is None:
                    _I._warn_once("progressive-torch", "umnn_amd: umnn_made_step does not cover this conditioner (weight dtype, more than 8 "
                                  "hidden layers or more new units in one step than its LDS hand-off holds): the progressive walk runs in "
                                  "torch ops.")
                walk = plan.walk(x_inv, context, use_kernel)

                def embed_progressive(j, widen):
                    h = walk.step(j)
                    return h.float().contiguous() if widen and h.dtype != torch.float32 else h
                return embed_progressive
        restrict = (rows_ok and context is None and not isinstance(made, ConditionnalMADE)
                    and self.net.embedding_dtype in (None, torch.float32) and os.environ.get("UMNN_INVERT_ROWS", "1") != "0")
        rows_all = (torch.arange(E, device=dev) * d).view(1, E) + torch.arange(d, device=dev).view(d, 1) if restrict else None
        h_buf = None

        def embed(j, widen):
            nonlocal restrict, h_buf
            hj = made.raw_rows(x_inv, rows_all[j]) if restrict else None
            if hj is not None:
                if h_buf is None:
                    h_buf = torch.zeros(B, E * d, device=dev)
                h_buf.view(B, E, d)[:, :, j] = hj
                return h_buf
            restrict = False
            h = self.net.make_embeding(x_inv, context)
            return h.float().contiguous() if widen else h
        return embed

    def _invert_newton(self, z, context=None, tol=1e-6, max_iter=64, conditioner="full", want_lj=False, lj=None):
        """``invert(method="newton")``.  HIP path: d x (conditioner + ONE launch), the whole solve of a dimension inside the kernel,
        writing x_inv[:, j] in place; nets the solve kernels do not cover, host tensors and other dtypes run the same iteration
        from the host (``integral.newton_solve``), one quadrature launch (or ATen quadrature) per iteration.
        ``want_lj`` -> (x, lj): the block's log-Jacobian row sum at x added to ``lj`` [B] (None: a fresh sum) -- in the solve launch
        itself (``umnn_cc_solve_lj``) on the HIP path, from ``newton_solve``'s f(x) in the tensors' dtype otherwise."""
        B, d = z.shape
        dev = z.device
        integrand = self.net.parallel_nets
        spec = mlp_spec(integrand)
        in_kernel = (_I._use_hip(spec, z) and z.dtype == torch.float32 and self.nb_steps >= 1 and B > 0 and self.solver in _SOLVERS)
        with torch.no_grad():
            z = z.contiguous()
            x_inv = torch.zeros(B, d, device=dev, dtype=z.dtype)
            scaling = self.scaling.detach().float().contiguous()
            embed = self._dim_embedding(x_inv, context, in_kernel, conditioner)
            for j in range(self.input_size):
                h = embed(j, in_kernel)             # (umnn_cc_solve reads an fp32 embedding)
                if in_kernel:
                    lj_row, lj_first = None, False
                    if want_lj:
                        lj_first = lj is None or lj.dtype != torch.float32 or not lj.is_contiguous()
                        lj_row = torch.empty(B, device=dev, dtype=torch.float32) if lj_first else lj
                    if _I.hip_solve(spec, h, z, self.nb_steps, j=j, scaling=scaling, off_h0=True, lo=-50., hi=50., tol=tol,
                                    max_iter=max_iter, x_out=x_inv, want_info=False, lj_row=lj_row, lj_first=lj_first) is not None:
                        if lj_first:
                            lj = lj_row if lj is None else lj + lj_row
                        continue
                    in_kernel = False
                h_j = h.view(B, h.shape[1] // d, d)[:, :, j].to(z.dtype).contiguous()          # [B,E]; row 0 doubles as the offset

                def eval_fn(xc, h_j=h_j):
                    if _I._use_hip(spec, xc):
                        F, fx, _ = _I.hip_forward(spec, None, xc, h_j, self.nb_steps)
                        return F, fx
                    return self._conditional_integral(xc, h_j), integrand.independant_forward(torch.cat((xc, h_j), 1))

                x_j, f_j, st_j = _I.newton_solve(eval_fn, z[:, [j]], torch.exp(self.scaling[j]).to(z.dtype), h_j[:, [0]], -50., 50., tol, max_iter)
                x_inv[:, j] = x_j[:, 0]
                if want_lj:
                    lj_j = torch.log(f_j[:, 0] + 1e-10) + self.scaling[j].to(z.dtype)
                    lj_j = torch.where((st_j[:, 0] & _I._lib.SOLVE_NONFINITE) != 0, torch.full_like(lj_j, float("nan")), lj_j)
                    lj = lj_j if lj is None else lj + lj_j
        return (x_inv, lj) if want_lj else x_inv

    def _invert_jacobi(self, z, context=None, tol=1e-6, max_iter=64, sweep_tol=1e-6, max_sweeps=None, want_info=False, moves=None,
                       want_lj=False, lj=None):
        """``invert(method="jacobi")``: x <- 0; repeat { h <- conditioner(x); x_i <- solve_i(z_i; h) for EVERY i }.  The conditioner is
        autoregressive, so dimension i is final once x_<i are: after sweep t the first t dimensions hold the sequential answer, d sweeps
        reproduce ``method="newton"``, and a fixed point is the inverse.  HIP path: per sweep one conditioner pass and ONE launch over the
        B d rows (``umnn_cc_solve_block``), every sweep after the first warm-started from the previous x; host tensors, other dtypes
        and nets the solve kernels do not cover run the same sweeps through ``integral.newton_solve`` over [B, d].
        Stops when max |x_new - x| / max(1, |x_new|) <= ``sweep_tol`` (one scalar device-to-host read per sweep; ``sweep_tol`` = 0: no
        test and no read), in any case after ``max_sweeps`` sweeps (default d).  -> (x, info); info (``want_info``) = {"sweeps",
        "converged": the test was met or d sweeps ran, "status": the last sweep's status words [B,d], "max_evals": per sweep}.
        ``moves`` (a list; graphs.GraphedSampler): gets this block's max |x_K - x_{K-1}| / max(1, |x_K|) of the last sweep appended,
        as a 0-dim device tensor, without a host read.
        ``want_lj`` -> (x, info, lj): the sweeps also write their f_x (the same launch) and the last sweep's row sums of
        log(f_x + 1e-10) + s are added to ``lj`` [B] (None: a fresh sum) by one ``umnn_flow_sample_lj_rows`` launch -- the last sweep
        solved every dimension under the embedding of x_{K-1}, so the sum is the block's log-Jacobian at the returned x to the same
        order as x itself is the inverse."""
        B, d = z.shape
        dev = z.device
        integrand = self.net.parallel_nets
        spec = mlp_spec(integrand)
        use_hip = _I._use_hip(spec, z) and self.nb_steps >= 1 and self.solver in _SOLVERS
        in_kernel = use_hip and z.dtype == torch.float32 and B > 0
        max_sweeps = d if max_sweeps is None else int(max_sweeps)
        if max_sweeps < 1:
            raise ValueError("umnn_amd: invert(method='jacobi') needs max_sweeps >= 1")
        with torch.no_grad():
            z = z.contiguous()
            x = torch.zeros(B, d, device=dev, dtype=z.dtype)
            scaling = self.scaling.detach().float().contiguous()
            sweeps, met, status, evals, x_prev, fx = 0, False, None, [], x, None
            for sweep in range(max_sweeps):
                h = self.net.make_embeding(x, context)
                x_init = x if sweep > 0 else None
                out = None
                if in_kernel:
                    # (umnn_cc_solve_block reads an fp32 embedding; widening bf16 is exact)
                    out = _I.hip_solve_block(spec, h.float().contiguous(), z, self.nb_steps, scaling=scaling, off_h0=True, x_init=x_init,
                                             lo=-50., hi=50., tol=tol, max_iter=max_iter, want_info=want_info or want_lj)
                    in_kernel = out is not None
                if out is None:
                    def eval_fn(xc, h=h):
                        if use_hip and xc.dtype == torch.float32:
                            F, fx, _ = _I.hip_forward(spec, None, xc, h, self.nb_steps)
                            return F, fx
                        hh = h.to(xc.dtype)
                        return _I.aten_forward(integrand, torch.zeros_like(xc), xc, hh, self.nb_steps), integrand(xc, hh)
                    off = h.view(B, h.shape[1] // d, d)[:, 0, :].to(z.dtype)
                    out = _I.newton_solve(eval_fn, z, torch.exp(self.scaling).to(z.dtype).unsqueeze(0), off, -50., 50., tol, max_iter,
                                          x_init=x_init)
                x_new, fx, status = out
                sweeps += 1
                if want_info:
                    evals.append((status & _I._lib.SOLVE_EVALS_MASK).max() if B > 0 else torch.zeros((), dtype=torch.int32, device=dev))
                if sweep_tol > 0:
                    moved = (x_new - x).abs() > sweep_tol * x_new.abs().clamp(min=1.)      # (a NaN row never counts as moving)
                    met = not bool(moved.any())
                x_prev, x = x, x_new
                if met:
                    break
            if moves is not None:
                moves.append(((x - x_prev).abs() / x.abs().clamp(min=1.)).max())
            if want_lj:
                # an entry that ended non-finite returns x = NaN while its f_x is the last iterate's: its row's sum is NaN as well
                fx = torch.where(torch.isnan(x), x, fx)
                lj = _I.sample_lj_rows(fx.contiguous(), scaling if fx.dtype == torch.float32 else self.scaling.detach(), lj)
        info = None
        if want_info:
            info = {"sweeps": sweeps, "converged": bool(met or sweeps >= d), "status": status,
                    "max_evals": [int(e) for e in torch.stack(evals).tolist()]}
        return (x, info, lj) if want_lj else (x, info)

    def _invert_block_recorded(self, z, context, tol, max_iter, sweeps, want_lj=False):
        """One block of ``invert`` as a graph records it (caller: ``_invert_recorded``, under no_grad) -> (x, status, last_move, lj).
        ``want_lj``: lj [B] = the row sum of log(f_x + 1e-10) + s, composed in torch ops from the f_x the solve ops return (the newton
        form adds one column per step, the jacobi form sums the last sweep's f_x); None otherwise.
        The conditioner runs in its graph-mode composition with every mask product formed ONCE for the whole block inversion; scale
        and offset are folded into the target by torch ops, t = z exp(-s) - h[:, 0, :], as ``MonotonicNN.inverse`` does.
        ``sweeps`` None ("newton"): input_size steps of conditioner + ``umnn::cc_solve`` on the [B, 1] column -- the loop unrolls at
        trace time, so this is for small d; wide blocks record "jacobi".  ``sweeps`` = K ("jacobi"): K x (conditioner +
        ``umnn::cc_solve_block`` warm-started from the previous sweep), no test between them."""
        B = z.shape[0]
        d = self.input_size
        net_args = _I.spec_args(_I._hip_spec(self.net.parallel_nets, z, True))
        weights = self.net.made.graph_weights()
        n, tol, max_iter = int(self.nb_steps), float(tol), int(max_iter)
        target = z * torch.exp(-self.scaling.detach().float()).unsqueeze(0)
        x = torch.zeros_like(z)
        s = self.scaling.detach().float()
        if sweeps is None:
            fxs = []
            for j in range(d):
                h_j = self.net.graph_embedding(x, context, weights).view(B, -1, d)[:, :, j]       # [B,E]; row 0 doubles as the offset
                x_j, fx_j, _ = torch.ops.umnn.cc_solve(target[:, j:j + 1] - h_j[:, :1].float(), h_j, *net_args, n, -50., 50., tol, max_iter)
                x = torch.cat((x[:, :j], x_j, x[:, j + 1:]), 1)
                if want_lj:
                    fxs.append(fx_j)
            lj = (torch.log(torch.cat(fxs, 1) + 1e-10) + s.unsqueeze(0)).sum(1) if want_lj else None
            return x, None, None, lj
        x_prev, status, fx = x, None, None
        for sweep in range(sweeps):
            h = self.net.graph_embedding(x, context, weights)
            t = target - h.view(B, -1, d)[:, 0, :].float()
            x_new, fx, status = torch.ops.umnn.cc_solve_block(t, h, x if sweep > 0 else None, *net_args, n, -50., 50., tol, max_iter)
            x_prev, x = x, x_new
        lj = (torch.log(fx + 1e-10) + s.unsqueeze(0)).sum(1) if want_lj else None
        return x, status, ((x - x_prev).abs() / x.abs().clamp(min=1.)).max(), lj

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

    def _base_noise(self, n, generator=None):
        """z ~ N(0, I), [n, d] on the block's device (drawn on the generator's own device when one is given)."""
        dev = self.pi.device
        z = torch.randn(int(n), self.input_size, generator=generator, dtype=self.scaling.dtype, device=dev if generator is None else generator.device)
        return z.to(dev)

    def sample_and_log_prob(self, n, context=None, generator=None, **solve_opts):
        """``UMNNMAFFlow.sample_and_log_prob`` for a single block -> (x [n, d], log_prob [n]); method "newton" by default, under no_grad.
        (The Gaussian term uses the drawn noise itself; ``compute_ll`` of a single block clamps its z to +-10 first.)"""
        return _sample_and_log_prob(self, n, context, generator, solve_opts)

    def _invert(self, z, iter=10, context=None, conditioner="full", want_lj=False, lj=None):
        """``invert(method="bracket")`` -> x, or with ``want_lj`` (x, lj): the search never evaluates f(x), so this is the one method
        that pays a pass for the log-Jacobian -- one forward launch of the block's integrand at the result (f(x) is node 0 of a
        one-step quadrature, as in ``compute_log_jac``) under the embedding the search's last dimension left, which is the embedding of
        the result (the conditioner is autoregressive: every column was final when it was computed), so no conditioner pass more; its
        row sums are added to ``lj`` [B] (None: a fresh sum)."""
        x, h = self._bracket_search(z, iter, context, conditioner)
        if not want_lj:
            return x
        with torch.no_grad():
            integrand = self.net.parallel_nets
            spec = _I._hip_spec(integrand, x)
            if spec is not None and h.is_cuda:
                fx = _I.cc_forward_jac(spec, integrand, None, x, h, 1, True)[1]
            else:
                dt = self.scaling.dtype         # (the search returns fp32 whatever the block's dtype is)
                fx = integrand(x.to(dt), h.to(dt))
            scaling = self.scaling.detach()
            return x, _I.sample_lj_rows(fx.contiguous(), scaling.float().contiguous() if fx.dtype == torch.float32 else scaling, lj)

    def _bracket_search(self, z, iter, context, conditioner):
        """The search of ``_invert`` -> (x, h): h the embedding the last dimension was searched under."""
        K = 10
        B, d = z.shape
        dev = z.device
        spec = mlp_spec(self.net.parallel_nets)
        if (_I._use_hip(spec, z) and z.dtype == torch.float32 and self.nb_steps >= 1 and iter >= 1 and B > 0
                and self.solver in _SOLVERS):
            # d x (conditioner + ONE launch): the whole 10-way / `iter`-round search of a dimension runs inside the kernel
            with torch.no_grad():
                z = z.contiguous()
                x_inv = torch.zeros(B, d, device=dev)
                scaling = self.scaling.detach().float().contiguous()
                done = True
                embed = self._dim_embedding(x_inv, context, True, conditioner)
                for j in range(self.input_size):
                    h = embed(j, True)              # (umnn_flow_invert_dim reads an fp32 embedding: it has no umnn_io descriptor)
                    if not _I.hip_invert_dim(spec, h, z, scaling, self.nb_steps, j, iter, x_inv):
                        done = False
                        break
            if done:
                return x_inv, h
        frac = torch.linspace(0., 1., K, device=dev).view(K, 1)
        x_inv = torch.zeros(B, d, device=dev)
        scale = torch.exp(self.scaling)
        rows = torch.arange(B, device=dev)
        with torch.no_grad():
            embed = self._dim_embedding(x_inv, context, False, conditioner) if conditioner != "full" else None
            for j in range(self.input_size):
                h = self.net.make_embeding(x_inv, context) if embed is None else embed(j, False)
                h3 = h.view(B, h.shape[1] // d, d)
                h_j = h3[:, :, j]                                   # [B,E]; row 0 doubles as the offset
                offset = h_j[:, 0]
                h_rep = h_j.unsqueeze(0).expand(K, -1, -1).reshape(K * B, -1)
                left = torch.full((B,), -50., device=dev)
                right = torch.full((B,), 50., device=dev)
                best = torch.zeros(B, device=dev)
                for _ in range(iter):
                    cand = frac * (right - left).unsqueeze(0) + left.unsqueeze(0)          # [K,B]
                    F = self._conditional_integral(cand.reshape(-1, 1), h_rep).view(K, B)
                    z_est = scale[j] * (offset.unsqueeze(0) + F)
                    m = torch.abs(z_est - z[:, j].unsqueeze(0)).argmin(0)                  # [B]
                    below = z_est[m, rows] < z[:, j]
                    lo = cand[(m - 1).clamp(min=0), rows]
                    hi = cand[(m + 1).clamp(max=K - 1), rows]
                    best = cand[m, rows]
                    left = torch.where(below, best, lo)
                    right = torch.where(below, hi, best)
                x_inv[:, j] = best
        return x_inv, h


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
        return _invert_dispatch(UMNNMAFFlow, self, z, iter, context, method, tol, max_iter, sweep_tol, max_sweeps, return_info, conditioner,
                                return_log_jac)

    def _invert_newton(self, z, context=None, tol=1e-6, max_iter=64, conditioner="full", want_lj=False):
        z = torch.flip(z, [1])
        lj = None
        for i in range(len(self.nets) - 1, -1, -1):
            if want_lj:
                z, lj = self.nets[i]._invert_newton(torch.flip(z, [1]), context, tol, max_iter, conditioner, True, lj)
            else:
                z = self.nets[i].invert(torch.flip(z, [1]), context=context, method="newton", tol=tol, max_iter=max_iter, conditioner=conditioner)
        return (z, lj) if want_lj else z

    def _invert_jacobi(self, z, context=None, tol=1e-6, max_iter=64, sweep_tol=1e-6, max_sweeps=None, want_info=False, moves=None,
                       want_lj=False):
        nb = len(self.nets)
        infos = [None] * nb
        z = torch.flip(z, [1])
        lj = None
        for i in range(nb - 1, -1, -1):
            out = self.nets[i]._invert_jacobi(torch.flip(z, [1]), context, tol, max_iter, sweep_tol, max_sweeps, want_info, moves, want_lj, lj)
            z, infos[i] = out[0], out[1]
            if want_lj:
                lj = out[2]
        info = {k: [inf[k] for inf in infos] for k in ("sweeps", "converged", "status", "max_evals")} if want_info else None
        return (z, info, lj) if want_lj else (z, info)

    def inverse(self, z, context=None, method="newton", tol=1e-6, max_iter=64, sweep_tol=1e-6, max_sweeps=None, adj_tol=1e-6,
                max_adj_sweeps=None, return_info=False):
        """The sampling direction with gradients to z, every parameter and the context: ``UMNNMAF.inverse`` block by block, walking
        the blocks and flipping as ``invert(method="newton")`` does (the flips are ordinary differentiable ops).  ``return_info=True``
        -> (x, info) with info["solve"] / info["adjoint"] as lists over the blocks in flow order; the backward fills info["adjoint"]."""
        return _inv.inverse(self.nets, True, "UMNNMAFFlow.inverse", z, context, method, tol, max_iter, sweep_tol, max_sweeps, adj_tol,
                            max_adj_sweeps, return_info)

    def _base_noise(self, n, generator=None):
        """z ~ N(0, I), [n, d] on the model's device (drawn on the generator's own device when one is given)."""
        blk = self.nets[0]
        dev = self.pi.device
        z = torch.randn(int(n), blk.input_size, generator=generator, dtype=blk.scaling.dtype,
                        device=dev if generator is None else generator.device)
        return z.to(dev)

    def sample(self, n, context=None, generator=None, **solve_opts):
        """n samples x = T^-1(z), z ~ N(0, I), without a graph: ``invert`` (method "newton" unless ``solve_opts`` says otherwise).
        Recorded by torch.compile / torch.export where ``invert`` is, when no generator is given."""
        solve_opts.setdefault("method", "newton")
        with torch.no_grad():
            return self.invert(self._base_noise(n, generator), context=context, **solve_opts)

    def rsample(self, n, context=None, generator=None, **opts):
        """n reparameterised samples: ``inverse`` of z ~ N(0, I), differentiable in the parameters and the context."""
        return self.inverse(self._base_noise(n, generator), context=context, **opts)

    def sample_and_log_prob(self, n, context=None, generator=None, **solve_opts):
        """n samples with their log-density -> (x [n, d], log_prob [n]): ``sample`` whose solves also hand over f(x), the diagonal of
        every block's Jacobian (``invert(..., return_log_jac=True)``), so that
            log q(x) = sum_blocks sum_i [log(f(x_i) + 1e-10) + s_i] - 1/2 sum_i (log 2 pi + z_i^2),   z the noise x was drawn from,
        ``compute_ll``'s formula term by term, costs no second conditioner and quadrature pass (``sample`` + ``log_prob(x)`` runs
        both again); the Gaussian term is one ``umnn_flow_sample_ll`` launch, or the same arithmetic in torch ops off the HIP path
        and in recorded graphs.  x is the x of ``sample`` with the same generator state and options.  It differs from ``log_prob(x)``
        by the solve's residual only (z against T(x): at most ``tol`` max(1, |z|) per dimension).  Runs under no_grad: a density to
        differentiate is ``log_prob(x)``, and reparameterised samples come from ``rsample``."""
        return _sample_and_log_prob(self, n, context, generator, solve_opts)

    def log_prob(self, x, context=None):
        return self.compute_ll(x, context)[0]

    def _invert(self, z, iter=10, context=None, conditioner="full", want_lj=False):
        z = torch.flip(z, [1])
        lj = None
        for i in range(len(self.nets) - 1, -1, -1):
            if want_lj:
                z, lj = self.nets[i]._invert(torch.flip(z, [1]), iter, context, conditioner, True, lj)
            else:
                z = self.nets[i].invert(torch.flip(z, [1]), iter, context=context, conditioner=conditioner)
        return (z, lj) if want_lj else z

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
