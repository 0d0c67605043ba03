"""The HIP entry points as ``torch.library`` custom ops (namespace ``umnn``): what torch.compile, torch.export and
torch.jit.trace record instead of the ctypes calls they cannot see.

    umnn::cc_forward(x0?, x, h, W[], b[], hidden_act, out_act, nb_steps, inv_f) -> (F, f_x)
    umnn::cc_backward(x0?, x, h, g, g_fx?, W[], b[], hidden_act, out_act, nb_steps, need[4], inv_f) -> (dx0, dx, dh, dtheta)
    umnn::cc_forward_multi(x0?, x, h, W[], b[], hidden_act, out_act, nb_steps, inv_f) -> (F, f_x)        x [B,1]; F, f_x [B, n_out]
    umnn::cc_forward_multi_nodes(x0?, x, h, W[], b[], hidden_act, out_act, nb_steps) -> (F, f_nodes)    x [B,1]; n_out = 1..16;
        F [B, n_out], f_nodes [B, nb_steps + 1, n_out]: the integrand at every node, node 0 = x
    umnn::cc_cumulate(values, x0?, x, nb_steps, ascending=False) -> out       values, out [B, nb_steps + 1, K]; x [B,1]: the integral
        from x0 up to every node, ascending from the lower limit; ``ascending``: values are stored that way too (else in node order)
    umnn::cc_backward_multi_nodes(x0?, x, h, cot_nodes, W[], b[], hidden_act, out_act, nb_steps, need[4]) -> (dx0_tau, dx_tau, dh, dtheta)
        x [B,1]; n_out = 1..16; cot_nodes [B, nb_steps + 1, n_out]: a cotangent per node, node 0 = x (``integral.hip_backward_multi_nodes``)
    umnn::cc_cumulate_adjoint(g, nb_steps, ascending=False) -> out       g, out [B, nb_steps + 1, K]: the adjoint of cc_cumulate without
        its span factor; out in node order, or -- ``ascending`` -- from the lower limit up
    umnn::cc_backward_multi(x0?, x, h, g, W[], b[], hidden_act, out_act, nb_steps, need[4], inv_f) -> (dx0, dx, dh, dtheta)
    umnn::cc_backward_multi_fx(x0?, x, h, g, g_fx?, W[], b[], hidden_act, out_act, nb_steps, need[4], inv_f) -> (dx0, dx, dh, dtheta)
    umnn::cc_solve(t, h, W[], b[], hidden_act, out_act, nb_steps, lo, hi, tol, max_iter) -> (x, f_x, status)
    umnn::cc_solve_block(t, h, x_init?, W[], b[], hidden_act, out_act, nb_steps, lo, hi, tol, max_iter) -> (x, f_x, status)
    umnn::cc_solve_multi(t, coef, h, W[], b[], hidden_act, out_act, nb_steps, lo, hi, tol, max_iter) -> (x, F, f_x, status)
        t, x, status [B,1]; coef, F, f_x [B, n_out]: x with sum_k coef_k int_0^x f_k = t
    umnn::flow_block(x, h, scaling, W[], b[], hidden_act, out_act, nb_steps, reverse_z, log_jac_in?) -> (z, log_jac, f_x)
    umnn::flow_block_backward(x, h, scaling, f_x, gz, glj, W[], b[], hidden_act, out_act, nb_steps, reverse_z, need[3])
        -> (dx, dh, dtheta)
    umnn::flow_ll(z, log_jac) -> ll
    umnn::flow_ll_backward(z, g_ll) -> (gz, glj)
    umnn::flow_ll_block(x, h, scaling, W[], b[], hidden_act, out_act, nb_steps, reverse_z, first, last, ll_in?) -> (z, ll)

The integrand crosses the op boundary as tensors and plain values -- the fields of ``nets.MlpSpec`` -- never as a module.  Every
implementation calls the eager path's own ``integral.hip_*`` function (same arithmetic mode, overflow fallback and
``path_taken()`` bookkeeping); every output is a fresh tensor and no op writes an input.  Outputs an op is told it need not
compute (``need``) come back as empty tensors.  cc_forward, cc_forward_multi, flow_block and flow_ll are differentiable (their
backward is the matching op -- cc_forward_multi's is cc_backward_multi_fx when a cotangent for its f_x output arrives, cc_backward_multi
when none does; cc_solve -- x with int_0^x f = t, ``integral.solve_integral`` -- is differentiable in its x output through cc_backward,
by the implicit-function theorem; cc_solve_multi -- ``integral.solve_sum`` -- likewise, in t, coef, h and the weights, through
cc_backward_multi; cc_solve_block -- the same solve for every (row, dimension) in ONE launch, optionally warm-started,
what the recorded ``invert(method="jacobi")`` sweeps call under no_grad -- has no autograd formula: a backward through it raises, as
it does through cc_forward_multi_nodes and cc_cumulate, the launches of the curves (``integral.CurveFunction`` /
``integral.CumulateFunction`` own their backward and record it as cc_cumulate_adjoint and cc_backward_multi_nodes; otherwise
``integral.IntegralCurve`` runs ATen under autograd);
flow_block's f_x output is not differentiable and its ``scaling`` must be frozen); the backward ops and
flow_ll_block are not.  Registration loads no library and touches no GPU.

The ops are public, so every real and fake implementation first checks what it was given (``_check_*``): one CUDA device for
every tensor, an integrand the kernels take (fp32 weights, the widths ``nets.mlp_spec`` accepts), x [B,d] / h [B,E*d] and the
shapes of the other operands against them, and fp32 where the entry point is fp32-only.  Anything else raises a RuntimeError --
at trace time through the fakes -- before a pointer reaches the kernels.
"""
from typing import List, Optional

import torch
import torch.nn.functional as F
from torch import Tensor

from . import _lib
from . import integral as _I
from .nets import spec_from_tensors

_FLOATS = (torch.float32, torch.bfloat16, torch.float16)
_F32 = (torch.float32,)


# ---------------------------------------------------------------------------------------------------------- argument checks
def _req(op, cond, msg):
    torch._check(cond, lambda: f"umnn::{op}: {msg}")


def _check_tensor(op, name, t, x, shape, dtypes):
    """``t`` on x's device, of ``shape`` (a tuple that may hold x's symbolic sizes) and one of ``dtypes``."""
    _req(op, t.device == x.device, f"{name} is on {t.device}, x on {x.device}")
    _req(op, t.dtype in dtypes, f"{name} has dtype {t.dtype}; expected {' or '.join(str(d) for d in dtypes)}")
    _req(op, t.dim() == len(shape), f"{name} has {t.dim()} dimensions; expected {len(shape)}")
    for i, n in enumerate(shape):
        _req(op, t.shape[i] == n, f"{name} has shape {tuple(t.shape)}; expected {tuple(shape)}")


def _check_net(op, x, h, W, b, hidden_act, out_act, x_dtypes=_FLOATS, h_dtypes=_FLOATS, multi=False, min_out=2):
    """x [B,d] and h [B,E*d] on one CUDA device, W[] / b[] an integrand MLP the kernels take (the rules of
    nets._spec_from_sequential) on that device.  ``multi``: the multi-output ops -- a last layer of ``min_out``..16 outputs and x [B,1];
    every other op takes exactly one output.  -> (B, d)."""
    _req(op, x.device.type == "cuda", f"x is on {x.device}; the HIP kernels need CUDA tensors")
    _req(op, x.dim() == 2, f"x has shape {tuple(x.shape)}; expected [B, d]")
    _req(op, x.dtype in x_dtypes, f"x has dtype {x.dtype}; expected {' or '.join(str(d) for d in x_dtypes)}")
    _req(op, len(W) == len(b) and 2 <= len(W) <= _lib.MAX_LINEAR,
         f"the integrand needs 2 to {_lib.MAX_LINEAR} layers with one bias each (got {len(W)} weights, {len(b)} biases)")
    _req(op, hidden_act in (_lib.ACT_LEAKY_RELU, _lib.ACT_RELU), f"unknown hidden_act {hidden_act}")
    _req(op, out_act in (_lib.OUT_ELU_PLUS_ONE, _lib.OUT_SIGMOID), f"unknown out_act {out_act}")
    for l, (w, bb) in enumerate(zip(W, b)):
        _req(op, w.dim() == 2 and bb.dim() == 1 and bb.shape[0] == w.shape[0],
             f"layer {l}: W {tuple(w.shape)} and b {tuple(bb.shape)} are not [out, in] and [out]")
        for name, t in ((f"W[{l}]", w), (f"b[{l}]", bb)):
            _req(op, t.device == x.device, f"{name} is on {t.device}, x on {x.device}")
            _req(op, t.dtype == torch.float32, f"{name} has dtype {t.dtype}; the integrand weights must be fp32")
        if l > 0:
            _req(op, w.shape[1] == W[l - 1].shape[0], f"layer {l} takes {w.shape[1]} inputs, layer {l - 1} gives {W[l - 1].shape[0]}")
        if l + 1 < len(W):
            _req(op, w.shape[0] <= 127, f"hidden layer {l} has {w.shape[0]} units; the kernels take at most 127")
    if multi:
        _req(op, min_out <= W[-1].shape[0] <= _lib.MAX_OUTPUTS,
             f"the integrand's last layer has n_out = {W[-1].shape[0]} outputs; expected {min_out} to {_lib.MAX_OUTPUTS}")
        _req(op, x.shape[1] == 1, f"x has shape {tuple(x.shape)}; a multi-output integrand is integrated over x [B, 1]")
    else:
        _req(op, W[-1].shape[0] == 1, f"the integrand's last layer has {W[-1].shape[0]} outputs; expected 1 (n_out = 1)")
    E = W[0].shape[1] - 1
    _req(op, E >= 1, "the integrand's first layer takes fewer than 2 inputs")
    B, d = x.shape
    _check_tensor(op, "h", h, x, (B, E * d), h_dtypes)
    return B, d


def _check_need(op, need, n):
    _req(op, len(need) == n, f"need has {len(need)} entries; expected {n}")


def _check_cc(op, x0, x, h, W, b, hidden_act, out_act, g=None, g_fx=None, need=None, multi=False):
    """The quadrature ops: x0 shaped like x; the cotangents [B, d], or [B, n_out] over x [B, 1] (``multi``); ``need`` of four."""
    B, d = _check_net(op, x, h, W, b, hidden_act, out_act, multi=multi)
    if x0 is not None:
        _check_tensor(op, "x0", x0, x, (B, 1) if multi else (B, d), _FLOATS)
    for name, t in (("g", g), ("g_fx", g_fx)):
        if t is not None:
            _check_tensor(op, name, t, x, (B, W[-1].shape[0]) if multi else (B, d), _FLOATS)
    if need is not None:
        _check_need(op, need, 4)


def _check_block(op, x, h, scaling, W, b, hidden_act, out_act, x_dtypes=_FLOATS, h_dtypes=_FLOATS, s_dtypes=_FLOATS):
    B, d = _check_net(op, x, h, W, b, hidden_act, out_act, x_dtypes, h_dtypes)
    _check_tensor(op, "scaling", scaling, x, (d,), s_dtypes)
    return B, d


def _check_solve(op, nb_steps, lo, hi, tol, max_iter):
    _req(op, nb_steps >= 1, f"nb_steps is {nb_steps}; expected >= 1")
    _req(op, lo < hi, f"empty bracket [{lo}, {hi}]")
    _req(op, tol >= 0, f"tol is {tol}; expected >= 0")
    _req(op, 1 <= max_iter <= _lib.SOLVE_EVALS_MASK, f"max_iter is {max_iter}; expected 1..{_lib.SOLVE_EVALS_MASK}")


def _check_flow_block(x, h, scaling, W, b, hidden_act, out_act, nb_steps, reverse_z, log_jac_in):
    B, d = _check_block("flow_block", x, h, scaling, W, b, hidden_act, out_act)
    if log_jac_in is not None:
        _check_tensor("flow_block", "log_jac_in", log_jac_in, x, (B, d), _FLOATS)


def _check_flow_block_backward(x, h, scaling, fx, gz, glj, W, b, hidden_act, out_act, nb_steps, reverse_z, need):
    # (umnn_flow_block_cotangents is fp32-only: f_x, the cotangents and scaling; the training block stores x in fp32)
    op = "flow_block_backward"
    B, d = _check_block(op, x, h, scaling, W, b, hidden_act, out_act, _F32, (torch.float32, torch.bfloat16), _F32)
    for name, t in (("fx", fx), ("gz", gz), ("glj", glj)):
        _check_tensor(op, name, t, x, (B, d), _F32)
    _check_need(op, need, 3)


def _check_z(op, z):
    # (umnn_flow_ll_forward / _backward are fp32-only)
    _req(op, z.device.type == "cuda", f"z is on {z.device}; the HIP kernels need CUDA tensors")
    _req(op, z.dim() == 2, f"z has shape {tuple(z.shape)}; expected [B, d]")
    _check_tensor(op, "z", z, z, tuple(z.shape), _F32)


def _check_flow_ll(z, log_jac):
    _check_z("flow_ll", z)
    _check_tensor("flow_ll", "log_jac", log_jac, z, tuple(z.shape), _F32)


def _check_flow_ll_backward(z, g_ll):
    _check_z("flow_ll_backward", z)
    _check_tensor("flow_ll_backward", "g_ll", g_ll, z, (z.shape[0],), _F32)


def _check_flow_ll_block(x, h, scaling, W, b, hidden_act, out_act, nb_steps, reverse_z, first, last, ll_in):
    # (umnn_flow_ll_block_forward is fp32-only: x, h, scaling and ll)
    B, d = _check_block("flow_ll_block", x, h, scaling, W, b, hidden_act, out_act, _F32, _F32, _F32)
    _req("flow_ll_block", first == (ll_in is None), "ll_in must be given exactly when first is False")
    if ll_in is not None:
        _check_tensor("flow_ll_block", "ll_in", ll_in, x, (B,), _F32)


# ---------------------------------------------------------------------------------------------------------- helpers
def _n_params(W, b):
    return sum(w.numel() for w in W) + sum(bb.numel() for bb in b)


def _empty(like, dtype=None):
    return like.new_empty((0,), dtype=dtype)


def _param_grads(dtheta, W, b, need_W, need_b):
    """Flat d_theta -> ([dW_l], [db_l]) views (``integral.split_flat``), None where not needed."""
    grads = _I.split_flat(dtheta, [p.shape for pair in zip(W, b) for p in pair], [n for pair in zip(need_W, need_b) for n in pair])
    return grads[0::2], grads[1::2]


# ---------------------------------------------------------------------------------------------------------- quadrature
@torch.library.custom_op("umnn::cc_forward", mutates_args=(), device_types="cuda")
def cc_forward(x0: Optional[Tensor], x: Tensor, h: Tensor, W: List[Tensor], b: List[Tensor], hidden_act: int, out_act: int,
               nb_steps: int, inv_f: bool) -> tuple[Tensor, Tensor]:
    _check_cc("cc_forward", x0, x, h, W, b, hidden_act, out_act)
    F_, fx, _ = _I.hip_forward(spec_from_tensors(W, b, hidden_act, out_act), x0, x, h, nb_steps, inv_f)
    return F_, fx


@cc_forward.register_fake
def _(x0, x, h, W, b, hidden_act, out_act, nb_steps, inv_f):
    _check_cc("cc_forward", x0, x, h, W, b, hidden_act, out_act)
    return x.new_empty(x.shape), x.new_empty(x.shape)


@torch.library.custom_op("umnn::cc_forward_multi", mutates_args=(), device_types="cuda")
def cc_forward_multi(x0: Optional[Tensor], x: Tensor, h: Tensor, W: List[Tensor], b: List[Tensor], hidden_act: int, out_act: int,
                     nb_steps: int, inv_f: bool) -> tuple[Tensor, Tensor]:
    """``integral.hip_forward_multi`` for an integrand given as tensors -> (F, f_x), each [B, n_out]; for the nets whose images
    exceed the LDS (``integral._multi_kernels_ok``, decided here at run time) the ATen quadrature on ``pure_mlp``."""
    _check_cc("cc_forward_multi", x0, x, h, W, b, hidden_act, out_act, multi=True)
    spec = spec_from_tensors(W, b, hidden_act, out_act)
    if _I._multi_kernels_ok(spec):
        F_, fx, _ = _I.hip_forward_multi(spec, x0, x, h, nb_steps, inv_f)
        return F_, fx
    f, params = pure_mlp(W, b, hidden_act, out_act)
    with torch.no_grad():
        xd, hd = x.detach(), h.detach()
        x0d = torch.zeros_like(xd) if x0 is None else x0.detach()
        return _I.aten_forward(lambda t, hh: f(params, t, hh), x0d, xd, hd, nb_steps, inv_f), f(params, xd, hd)


@cc_forward_multi.register_fake
def _(x0, x, h, W, b, hidden_act, out_act, nb_steps, inv_f):
    _check_cc("cc_forward_multi", x0, x, h, W, b, hidden_act, out_act, multi=True)
    shape = (x.shape[0], W[-1].shape[0])
    return x.new_empty(shape), x.new_empty(shape)


# ---- curves: the forward that keeps its node values, and the cumulative quadrature of values at the nodes (no autograd formula)
def _check_nodes(x0, x, h, W, b, hidden_act, out_act, nb_steps):
    op = "cc_forward_multi_nodes"
    B, _ = _check_net(op, x, h, W, b, hidden_act, out_act, multi=True, min_out=1)
    if x0 is not None:
        _check_tensor(op, "x0", x0, x, (B, 1), _FLOATS)
    _req(op, nb_steps >= 1, f"nb_steps is {nb_steps}; expected >= 1")


@torch.library.custom_op("umnn::cc_forward_multi_nodes", mutates_args=(), device_types="cuda")
def cc_forward_multi_nodes(x0: Optional[Tensor], x: Tensor, h: Tensor, W: List[Tensor], b: List[Tensor], hidden_act: int, out_act: int,
                           nb_steps: int) -> tuple[Tensor, Tensor]:
    """``integral.hip_forward_multi_nodes`` for an integrand given as tensors -> (F [B, n_out], f_nodes [B, nb_steps + 1, n_out], node
    order); for what the library turns away (``integral._curve_kernels_ok``, decided here at run time) ``integral.aten_curve`` on
    ``pure_mlp``."""
    _check_nodes(x0, x, h, W, b, hidden_act, out_act, nb_steps)
    spec = spec_from_tensors(W, b, hidden_act, out_act)
    if _I._curve_kernels_ok(spec, nb_steps):
        return _I.hip_forward_multi_nodes(spec, x0, x, h, nb_steps)
    f, params = pure_mlp(W, b, hidden_act, out_act)
    with torch.no_grad():
        xd, hd = x.detach(), h.detach()
        _, C, fa = _I.aten_curve(lambda t, hh: f(params, t, hh), torch.zeros_like(xd) if x0 is None else x0.detach(), xd, hd, nb_steps)
        return C[:, -1].contiguous(), fa.flip(1)


@cc_forward_multi_nodes.register_fake
def _(x0, x, h, W, b, hidden_act, out_act, nb_steps):
    _check_nodes(x0, x, h, W, b, hidden_act, out_act, nb_steps)
    K = W[-1].shape[0]
    return x.new_empty((x.shape[0], K)), x.new_empty((x.shape[0], nb_steps + 1, K))


def _check_cumulate(values, x0, x, nb_steps):
    op = "cc_cumulate"
    _req(op, values.device.type == "cuda", f"values is on {values.device}; the HIP kernels need CUDA tensors")
    _req(op, nb_steps >= 1, f"nb_steps is {nb_steps}; expected >= 1")
    _req(op, values.dim() == 3, f"values has shape {tuple(values.shape)}; expected [B, nb_steps + 1, K]")
    _check_tensor(op, "values", values, values, (values.shape[0], nb_steps + 1, values.shape[2]), _FLOATS)
    _req(op, 1 <= values.shape[2] <= _lib.MAX_OUTPUTS, f"values has K = {values.shape[2]} outputs; expected 1 to {_lib.MAX_OUTPUTS}")
    _check_tensor(op, "x", x, values, (values.shape[0], 1), _FLOATS)
    if x0 is not None:
        _check_tensor(op, "x0", x0, values, (values.shape[0], 1), _FLOATS)


@torch.library.custom_op("umnn::cc_cumulate", mutates_args=(), device_types="cuda")
def cc_cumulate(values: Tensor, x0: Optional[Tensor], x: Tensor, nb_steps: int, ascending: bool = False) -> Tensor:
    """``integral.hip_cumulate`` -> [B, nb_steps + 1, K] ascending; beyond the kernel's table budget (decided here at run time) the
    einsum of ``integral.aten_cumulate``."""
    _check_cumulate(values, x0, x, nb_steps)
    if _I._cumulate_kernel_ok(values.shape[2], nb_steps):
        return _I.hip_cumulate(values, x0, x, nb_steps, ascending)
    with torch.no_grad():
        return _I.aten_cumulate(values.detach(), x0, x, nb_steps, ascending)


@cc_cumulate.register_fake
def _(values, x0, x, nb_steps, ascending=False):
    _check_cumulate(values, x0, x, nb_steps)
    return values.new_empty(values.shape)


# ---- the backward of the curves: the adjoint of cc_cumulate and the multi-output backward with a cotangent per node
def _check_cumulate_adjoint(g, nb_steps):
    op = "cc_cumulate_adjoint"
    _req(op, g.device.type == "cuda", f"g is on {g.device}; the HIP kernels need CUDA tensors")
    _req(op, nb_steps >= 1, f"nb_steps is {nb_steps}; expected >= 1")
    _req(op, g.dim() == 3, f"g has shape {tuple(g.shape)}; expected [B, nb_steps + 1, K]")
    _check_tensor(op, "g", g, g, (g.shape[0], nb_steps + 1, g.shape[2]), _FLOATS)
    _req(op, 1 <= g.shape[2] <= _lib.MAX_OUTPUTS, f"g has K = {g.shape[2]} outputs; expected 1 to {_lib.MAX_OUTPUTS}")


@torch.library.custom_op("umnn::cc_cumulate_adjoint", mutates_args=(), device_types="cuda")
def cc_cumulate_adjoint(g: Tensor, nb_steps: int, ascending: bool = False) -> Tensor:
    """``integral.hip_cumulate_adjoint`` -> [B, nb_steps + 1, K]; beyond the kernel's table budget (decided here at run time) the
    einsum of ``integral.aten_cumulate_adjoint``."""
    _check_cumulate_adjoint(g, nb_steps)
    if _I._cumulate_kernel_ok(g.shape[2], nb_steps, adjoint=True):
        return _I.hip_cumulate_adjoint(g, nb_steps, ascending)
    with torch.no_grad():
        return _I.aten_cumulate_adjoint(g.detach(), nb_steps, ascending).contiguous()


@cc_cumulate_adjoint.register_fake
def _(g, nb_steps, ascending=False):
    _check_cumulate_adjoint(g, nb_steps)
    return g.new_empty(g.shape)


def _check_backward_nodes(x0, x, h, cot_nodes, W, b, hidden_act, out_act, nb_steps, need):
    op = "cc_backward_multi_nodes"
    B, _ = _check_net(op, x, h, W, b, hidden_act, out_act, multi=True, min_out=1)
    if x0 is not None:
        _check_tensor(op, "x0", x0, x, (B, 1), _FLOATS)
    _req(op, nb_steps >= 1, f"nb_steps is {nb_steps}; expected >= 1")
    _check_tensor(op, "cot_nodes", cot_nodes, x, (B, nb_steps + 1, W[-1].shape[0]), _FLOATS)
    _check_need(op, need, 4)


@torch.library.custom_op("umnn::cc_backward_multi_nodes", mutates_args=(), device_types="cuda")
def cc_backward_multi_nodes(x0: Optional[Tensor], x: Tensor, h: Tensor, cot_nodes: Tensor, W: List[Tensor], b: List[Tensor],
                            hidden_act: int, out_act: int, nb_steps: int, need: List[bool]) -> tuple[Tensor, Tensor, Tensor, Tensor]:
    """``integral.hip_backward_multi_nodes`` for an integrand given as tensors -> (dx0_tau, dx_tau, dh, dtheta), empty where not
    needed; for what the library turns away (``integral._curve_grad_kernels_ok``, decided here at run time) ``integral.aten_vjp_nodes``
    on ``pure_mlp``."""
    _check_backward_nodes(x0, x, h, cot_nodes, W, b, hidden_act, out_act, nb_steps, need)
    need = [bool(need[0]) and x0 is not None] + [bool(n) for n in need[1:]]
    spec = spec_from_tensors(W, b, hidden_act, out_act)
    if _I._curve_grad_kernels_ok(spec, nb_steps):
        out = _I.hip_backward_multi_nodes(spec, x0, x, h, cot_nodes, nb_steps, need)
    else:
        xd, hd = x.detach().float(), h.detach().float()
        out = _I.aten_vjp_nodes(pure_mlp(W, b, hidden_act, out_act), torch.zeros_like(xd) if x0 is None else x0.detach().float(), xd, hd,
                                cot_nodes.detach().float(), nb_steps)
        out = (out[0].to(x.dtype), out[1].to(x.dtype), out[2].to(h.dtype), out[3])
    like = (x, x, h, W[0])
    return tuple(t.contiguous() if (n and t is not None) else _empty(l, torch.float32 if i == 3 else None)
                 for i, (t, n, l) in enumerate(zip(out, need, like)))


@cc_backward_multi_nodes.register_fake
def _(x0, x, h, cot_nodes, W, b, hidden_act, out_act, nb_steps, need):
    _check_backward_nodes(x0, x, h, cot_nodes, W, b, hidden_act, out_act, nb_steps, need)
    return (x.new_empty(x.shape) if (need[0] and x0 is not None) else _empty(x),
            x.new_empty(x.shape) if need[1] else _empty(x),
            h.new_empty(h.shape) if need[2] else _empty(h),
            W[0].new_empty((_n_params(W, b),), dtype=torch.float32) if need[3] else _empty(W[0], torch.float32))


# The autograd glue of the two forward ops: one ctx layout, one ``need`` rule, one packer of the nine input gradients.
def _cc_setup(ctx, inputs, output):
    x0, x, h, W, b, hidden_act, out_act, nb_steps, inv_f = inputs
    ctx.meta = (hidden_act, out_act, nb_steps, inv_f, len(W), x0 is None)
    ctx.save_for_backward(*(() if x0 is None else (x0,)), x, h, *W, *b)


def _cc_saved(ctx):
    """-> ((x0, x, h), the integrand and step arguments every backward op ends in before ``need``, need[4])."""
    hidden_act, out_act, nb_steps, inv_f, L, x0_none = ctx.meta
    saved = ctx.saved_tensors
    x0, rest = (None, saved) if x0_none else (saved[0], saved[1:])
    nig = ctx.needs_input_grad
    need = [bool(nig[0]) and not x0_none, bool(nig[1]), bool(nig[2]), any(nig[3]) or any(nig[4])]
    return (x0, rest[0], rest[1]), (list(rest[2:2 + L]), list(rest[2 + L:]), hidden_act, out_act, nb_steps), need, inv_f


def _cc_input_grads(ctx, out, W, b, need):
    dx0, dx, dh, dtheta = out
    gW, gb = _param_grads(dtheta if need[3] else None, W, b, ctx.needs_input_grad[3], ctx.needs_input_grad[4])
    return (dx0 if need[0] else None, dx if need[1] else None, dh if need[2] else None, gW, gb,
            None, None, None, None)


def _cc_forward_backward(ctx, gF, gfx):
    lims, net, need, inv_f = _cc_saved(ctx)
    return _cc_input_grads(ctx, torch.ops.umnn.cc_backward(*lims, gF, gfx, *net, need, inv_f), net[0], net[1], need)


def _cc_forward_multi_setup(ctx, inputs, output):
    ctx.set_materialize_grads(False)               # (an f_x nobody differentiates: no zero cotangent, the backward of before)
    _cc_setup(ctx, inputs, output)


def _cc_forward_multi_backward(ctx, gF, gfx):
    if gF is None and gfx is None:
        return (None,) * 9
    (x0, x, h), net, need, inv_f = _cc_saved(ctx)
    gF = x.new_zeros((x.shape[0], net[0][-1].shape[0])) if gF is None else gF.contiguous()
    if gfx is None:
        out = torch.ops.umnn.cc_backward_multi(x0, x, h, gF, *net, need, inv_f)
    else:
        out = torch.ops.umnn.cc_backward_multi_fx(x0, x, h, gF, gfx.contiguous(), *net, need, inv_f)
    return _cc_input_grads(ctx, out, net[0], net[1], need)


cc_forward.register_autograd(_cc_forward_backward, setup_context=_cc_setup)
cc_forward_multi.register_autograd(_cc_forward_multi_backward, setup_context=_cc_forward_multi_setup)


def pure_mlp(W, b, hidden_act, out_act):
    """The integrand the ops get -- W[], b[] and the activation codes, never a module -- as ``integral.aten_vjp`` takes it:
    (f(params, x, h), params in parameters() order), f the MLP on the rows [x_i, h_{0,i}, ..., h_{E-1,i}]
    (nets.IntegrandNetwork.rows) -> [B, d] for one output, [B, n_out] for a multi-output last layer (x [B,1]: the rows are
    ``cat((x, h), 1)`` itself)."""
    L, n_in, n_out = len(W), W[0].shape[1], W[-1].shape[0]

    def f(params, x, h):
        B, d = x.shape
        a = torch.cat((x, h), 1).view(B, n_in, d).transpose(1, 2).reshape(B * d, n_in)
        for l in range(L):
            a = F.linear(a, params[2 * l], params[2 * l + 1])
            if l + 1 < L:
                a = F.leaky_relu(a, 0.01) if hidden_act == _lib.ACT_LEAKY_RELU else F.relu(a)
        return (F.elu(a) + 1. if out_act == _lib.OUT_ELU_PLUS_ONE else torch.sigmoid(a)).view(B, d * n_out)

    return f, [p.detach() for pair in zip(W, b) for p in pair]


def _cc_backward(op, multi, x0, x, h, g, g_fx, W, b, hidden_act, out_act, nb_steps, need, inv_f):
    """The three backward ops: ``integral.quadrature_backward`` for an integrand given as tensors -- the HIP kernels, or, for the
    nets ``integral._hip_backward_ok`` / ``_multi_kernels_ok`` turn away, decided here at run time, the one ATen backward on
    ``pure_mlp``."""
    _check_cc(op, x0, x, h, W, b, hidden_act, out_act, g, g_fx, need, multi)
    need = [bool(need[0]) and x0 is not None] + [bool(n) for n in need[1:]]
    out = _I.quadrature_backward(spec_from_tensors(W, b, hidden_act, out_act), pure_mlp(W, b, hidden_act, out_act), x0, x, h, g, g_fx,
                                 nb_steps, need, inv_f)
    like = (x, x, h, W[0])
    return tuple(t.contiguous() if (n and t is not None) else _empty(l, torch.float32 if i == 3 else None)
                 for i, (t, n, l) in enumerate(zip(out, need, like)))


def _cc_backward_fake(op, multi, x0, x, h, g, g_fx, W, b, hidden_act, out_act, nb_steps, need, inv_f):
    _check_cc(op, x0, x, h, W, b, hidden_act, out_act, g, g_fx, need, multi)
    return (x.new_empty(x.shape) if (need[0] and x0 is not None) else _empty(x),
            x.new_empty(x.shape) if need[1] else _empty(x),
            h.new_empty(h.shape) if need[2] else _empty(h),
            W[0].new_empty((_n_params(W, b),), dtype=torch.float32) if need[3] else _empty(W[0], torch.float32))


@torch.library.custom_op("umnn::cc_backward", mutates_args=(), device_types="cuda")
def cc_backward(x0: Optional[Tensor], x: Tensor, h: Tensor, g: Tensor, g_fx: Optional[Tensor], W: List[Tensor], b: List[Tensor],
                hidden_act: int, out_act: int, nb_steps: int, need: List[bool], inv_f: bool) -> tuple[Tensor, Tensor, Tensor, Tensor]:
    return _cc_backward("cc_backward", False, x0, x, h, g, g_fx, W, b, hidden_act, out_act, nb_steps, need, inv_f)


@torch.library.custom_op("umnn::cc_backward_multi", mutates_args=(), device_types="cuda")
def cc_backward_multi(x0: Optional[Tensor], x: Tensor, h: Tensor, g: Tensor, W: List[Tensor], b: List[Tensor],
                      hidden_act: int, out_act: int, nb_steps: int, need: List[bool], inv_f: bool) -> tuple[Tensor, Tensor, Tensor, Tensor]:
    """x [B,1], g [B, n_out] of a multi-output integrand: dx and dx0 [B,1] are sums over the outputs."""
    return _cc_backward("cc_backward_multi", True, x0, x, h, g, None, W, b, hidden_act, out_act, nb_steps, need, inv_f)


@torch.library.custom_op("umnn::cc_backward_multi_fx", mutates_args=(), device_types="cuda")
def cc_backward_multi_fx(x0: Optional[Tensor], x: Tensor, h: Tensor, g: Tensor, g_fx: Optional[Tensor], W: List[Tensor], b: List[Tensor],
                         hidden_act: int, out_act: int, nb_steps: int, need: List[bool], inv_f: bool) -> tuple[Tensor, Tensor, Tensor, Tensor]:
    """``cc_backward_multi`` with the cotangent ``g_fx`` [B, n_out] of the f_x output on top of ``g`` (None: exactly that op)."""
    return _cc_backward("cc_backward_multi_fx", True, x0, x, h, g, g_fx, W, b, hidden_act, out_act, nb_steps, need, inv_f)


@cc_backward.register_fake
def _(x0, x, h, g, g_fx, W, b, hidden_act, out_act, nb_steps, need, inv_f):
    return _cc_backward_fake("cc_backward", False, x0, x, h, g, g_fx, W, b, hidden_act, out_act, nb_steps, need, inv_f)


@cc_backward_multi.register_fake
def _(x0, x, h, g, W, b, hidden_act, out_act, nb_steps, need, inv_f):
    return _cc_backward_fake("cc_backward_multi", True, x0, x, h, g, None, W, b, hidden_act, out_act, nb_steps, need, inv_f)


@cc_backward_multi_fx.register_fake
def _(x0, x, h, g, g_fx, W, b, hidden_act, out_act, nb_steps, need, inv_f):
    return _cc_backward_fake("cc_backward_multi_fx", True, x0, x, h, g, g_fx, W, b, hidden_act, out_act, nb_steps, need, inv_f)


# ---------------------------------------------------------------------------------------------------------- inverse (Newton solve)
def _check_cc_solve(t, h, W, b, hidden_act, out_act, nb_steps, lo, hi, tol, max_iter):
    _check_net("cc_solve", t, h, W, b, hidden_act, out_act)
    _check_solve("cc_solve", nb_steps, lo, hi, tol, max_iter)


@torch.library.custom_op("umnn::cc_solve", mutates_args=(), device_types="cuda")
def cc_solve(t: Tensor, h: Tensor, W: List[Tensor], b: List[Tensor], hidden_act: int, out_act: int, nb_steps: int,
             lo: float, hi: float, tol: float, max_iter: int) -> tuple[Tensor, Tensor, Tensor]:
    """x [B,d] in [lo, hi] with int_0^x f(s; h) ds = t (``integral.solve_integral``: the in-kernel Newton solve, one launch per
    dimension), f(x; h) and the int32 status word per element.  The iteration count is data-dependent only inside the launch."""
    _check_cc_solve(t, h, W, b, hidden_act, out_act, nb_steps, lo, hi, tol, max_iter)
    return _I.solve_integral(spec_from_tensors(W, b, hidden_act, out_act), t, h, nb_steps, lo, hi, tol, max_iter)


@cc_solve.register_fake
def _(t, h, W, b, hidden_act, out_act, nb_steps, lo, hi, tol, max_iter):
    _check_cc_solve(t, h, W, b, hidden_act, out_act, nb_steps, lo, hi, tol, max_iter)
    return t.new_empty(t.shape), t.new_empty(t.shape), t.new_empty(t.shape, dtype=torch.int32)


def _cc_solve_setup(ctx, inputs, output):
    t, h, W, b, hidden_act, out_act, nb_steps = inputs[:7]
    ctx.mark_non_differentiable(output[1], output[2])
    ctx.meta = (hidden_act, out_act, nb_steps, len(W))
    ctx.save_for_backward(output[0], h, output[1], *W, *b)


def _cc_solve_backward(ctx, g_x, _gfx, _gstatus):
    """Implicit backward: g_t = g_x / f(x); (d_theta, d_h) of the integral up to x for the cotangent -g_x / f(x)."""
    hidden_act, out_act, nb_steps, L = ctx.meta
    x, h, fx, *Wb = ctx.saved_tensors
    W, b = Wb[:L], Wb[L:]
    nig = ctx.needs_input_grad
    need = [False, False, bool(nig[1]), any(nig[2]) or any(nig[3])]
    g_t = g_x / fx
    dh = dtheta = None
    if need[2] or need[3]:
        _, _, dh, dtheta = torch.ops.umnn.cc_backward(None, x, h, -g_t, None, W, b, hidden_act, out_act, nb_steps, need, False)
    gW, gb = _param_grads(dtheta if need[3] else None, W, b, nig[2], nig[3])
    return (g_t if nig[0] else None, dh if need[2] else None, gW, gb, None, None, None, None, None, None, None)


cc_solve.register_autograd(_cc_solve_backward, setup_context=_cc_solve_setup)


def _check_cc_solve_multi(t, coef, h, W, b, hidden_act, out_act, nb_steps, lo, hi, tol, max_iter):
    B, _ = _check_net("cc_solve_multi", t, h, W, b, hidden_act, out_act, multi=True)
    _check_tensor("cc_solve_multi", "coef", coef, t, (B, W[-1].shape[0]), _FLOATS)
    _check_solve("cc_solve_multi", nb_steps, lo, hi, tol, max_iter)


@torch.library.custom_op("umnn::cc_solve_multi", mutates_args=(), device_types="cuda")
def cc_solve_multi(t: Tensor, coef: Tensor, h: Tensor, W: List[Tensor], b: List[Tensor], hidden_act: int, out_act: int, nb_steps: int,
                   lo: float, hi: float, tol: float, max_iter: int) -> tuple[Tensor, Tensor, Tensor, Tensor]:
    """x [B,1] in [lo, hi] with sum_k coef[:, k] int_0^x f_k(s; h) ds = t (``integral.solve_sum``: ONE launch of the in-kernel
    Newton solve on the K-output quadrature), F_k and f_k [B, n_out] at that x and the int32 status word per row.  For the nets
    whose images exceed the LDS (``integral._multi_kernels_ok``, decided here at run time) the same iteration on the ATen
    quadrature of ``pure_mlp``."""
    _check_cc_solve_multi(t, coef, h, W, b, hidden_act, out_act, nb_steps, lo, hi, tol, max_iter)
    spec = spec_from_tensors(W, b, hidden_act, out_act)
    if _I._multi_kernels_ok(spec):
        return _I.solve_sum(spec, None, t, coef, h, nb_steps, lo, hi, tol, max_iter)
    f, params = pure_mlp(W, b, hidden_act, out_act)
    return _I.solve_sum(None, lambda x, hh: f(params, x, hh), t, coef, h, nb_steps, lo, hi, tol, max_iter)


@cc_solve_multi.register_fake
def _(t, coef, h, W, b, hidden_act, out_act, nb_steps, lo, hi, tol, max_iter):
    _check_cc_solve_multi(t, coef, h, W, b, hidden_act, out_act, nb_steps, lo, hi, tol, max_iter)
    shape = (t.shape[0], W[-1].shape[0])
    return t.new_empty(t.shape), t.new_empty(shape), t.new_empty(shape), t.new_empty(t.shape, dtype=torch.int32)


def _cc_solve_multi_setup(ctx, inputs, output):
    t, coef, h, W, b, hidden_act, out_act, nb_steps = inputs[:8]
    ctx.mark_non_differentiable(output[1], output[2], output[3])
    ctx.meta = (hidden_act, out_act, nb_steps, len(W))
    ctx.save_for_backward(output[0], h, coef, output[1], output[2], *W, *b)


def _cc_solve_multi_backward(ctx, g_x, _gF, _gfx, _gstatus):
    """Implicit backward: with D = sum_k coef_k f_k(x), g_t = g_x / D, g_coef = -g_t F_k(x); (d_theta, d_h) of the K integrals up to
    x for the cotangent -g_t coef, through cc_backward_multi."""
    hidden_act, out_act, nb_steps, L = ctx.meta
    x, h, coef, F_, fx, *Wb = ctx.saved_tensors
    W, b = Wb[:L], Wb[L:]
    nig = ctx.needs_input_grad
    need = [False, False, bool(nig[2]), any(nig[3]) or any(nig[4])]
    g_t = g_x / (coef * fx).sum(1, keepdim=True)
    dh = dtheta = None
    if need[2] or need[3]:
        _, _, dh, dtheta = torch.ops.umnn.cc_backward_multi(None, x, h, -g_t * coef, W, b, hidden_act, out_act, nb_steps, need, False)
    gW, gb = _param_grads(dtheta if need[3] else None, W, b, nig[3], nig[4])
    return (g_t if nig[0] else None, -g_t * F_ if nig[1] else None, dh if need[2] else None, gW, gb,
            None, None, None, None, None, None, None)


cc_solve_multi.register_autograd(_cc_solve_multi_backward, setup_context=_cc_solve_multi_setup)


def _check_cc_solve_block(t, h, x_init, W, b, hidden_act, out_act, nb_steps, lo, hi, tol, max_iter):
    # (umnn_cc_solve_block is fp32-only in t, x_init and x; a bf16 embedding is widened, which is exact)
    op = "cc_solve_block"
    B, d = _check_net(op, t, h, W, b, hidden_act, out_act, _F32)
    if x_init is not None:
        _check_tensor(op, "x_init", x_init, t, (B, d), _F32)
    _check_solve(op, nb_steps, lo, hi, tol, max_iter)


@torch.library.custom_op("umnn::cc_solve_block", mutates_args=(), device_types="cuda")
def cc_solve_block(t: Tensor, h: Tensor, x_init: Optional[Tensor], W: List[Tensor], b: List[Tensor], hidden_act: int, out_act: int,
                   nb_steps: int, lo: float, hi: float, tol: float, max_iter: int) -> tuple[Tensor, Tensor, Tensor]:
    """x [B,d] in [lo, hi] with int_0^x f(s; h[:, :, i]) ds = t[:, i] for EVERY (row, dimension) in one launch
    (``integral.hip_solve_block`` without scale and offset: the caller folds the flow's into t), started at ``x_init`` when given;
    f(x; h) and the int32 status word per element.  Nets outside the solve tables run ``integral.newton_solve`` over [B, d] on the
    forward kernel.  No autograd formula: the sweeps of ``invert`` run under no_grad."""
    _check_cc_solve_block(t, h, x_init, W, b, hidden_act, out_act, nb_steps, lo, hi, tol, max_iter)
    spec = spec_from_tensors(W, b, hidden_act, out_act)
    t32, h32 = t.detach().contiguous(), _I._f32c(h)
    x0 = None if x_init is None else x_init.detach().contiguous()
    with torch.no_grad():
        if t32.shape[0] == 0:
            return torch.empty_like(t32), torch.empty_like(t32), torch.empty(t32.shape, device=t32.device, dtype=torch.int32)
        out = _I.hip_solve_block(spec, h32, t32, nb_steps, scaling=None, off_h0=False, x_init=x0, lo=lo, hi=hi, tol=tol, max_iter=max_iter)
        if out is None:
            out = _I.host_solve(spec, h32, t32, nb_steps, lo, hi, tol, max_iter, x_init=x0)
    return out


@cc_solve_block.register_fake
def _(t, h, x_init, W, b, hidden_act, out_act, nb_steps, lo, hi, tol, max_iter):
    _check_cc_solve_block(t, h, x_init, W, b, hidden_act, out_act, nb_steps, lo, hi, tol, max_iter)
    return t.new_empty(t.shape), t.new_empty(t.shape), t.new_empty(t.shape, dtype=torch.int32)


# ---------------------------------------------------------------------------------------------------------- flow block
@torch.library.custom_op("umnn::flow_block", mutates_args=(), device_types="cuda")
def flow_block(x: Tensor, h: Tensor, scaling: Tensor, W: List[Tensor], b: List[Tensor], hidden_act: int, out_act: int,
               nb_steps: int, reverse_z: bool, log_jac_in: Optional[Tensor]) -> tuple[Tensor, Tensor, Tensor]:
    """One UMNN-MAF block: the fused-epilogue launch of ``hip_flow_block`` (no z_2 hand-off: a training backward recomputes it).
    f_x is returned for the backward and is not differentiable."""
    _check_flow_block(x, h, scaling, W, b, hidden_act, out_act, nb_steps, reverse_z, log_jac_in)
    z, lj, fx, _ = _I.hip_flow_block(spec_from_tensors(W, b, hidden_act, out_act), x, h, scaling, nb_steps, reverse_z, log_jac_in)
    return z, lj, fx


@flow_block.register_fake
def _(x, h, scaling, W, b, hidden_act, out_act, nb_steps, reverse_z, log_jac_in):
    _check_flow_block(x, h, scaling, W, b, hidden_act, out_act, nb_steps, reverse_z, log_jac_in)
    return x.new_empty(x.shape), x.new_empty(x.shape), x.new_empty(x.shape)


def _flow_block_setup(ctx, inputs, output):
    x, h, scaling, W, b, hidden_act, out_act, nb_steps, reverse_z, log_jac_in = inputs
    # (the terms of the backward below are those of a frozen scaling on fp32 storage: integral.fused_block_ok's conditions)
    if scaling.requires_grad:
        raise RuntimeError("umnn::flow_block: no gradient for a trainable scaling (UMNNMAF freezes it); use the composed path")
    if x.dtype != torch.float32:
        raise RuntimeError(f"umnn::flow_block: differentiable for fp32 x only (got {x.dtype})")
    ctx.mark_non_differentiable(output[2])
    ctx.meta = (hidden_act, out_act, nb_steps, reverse_z, len(W))
    ctx.save_for_backward(x, h, scaling, output[2], *W, *b)


def _flow_block_backward(ctx, gz, glj, _gfx):
    hidden_act, out_act, nb_steps, reverse_z, L = ctx.meta
    x, h, scaling, fx, *Wb = ctx.saved_tensors
    W, b = Wb[:L], Wb[L:]
    nig = ctx.needs_input_grad
    need = [bool(nig[0]), bool(nig[1]), any(nig[3]) or any(nig[4])]
    dx, dh, dtheta = torch.ops.umnn.flow_block_backward(x, h, scaling, fx, gz, glj, W, b, hidden_act, out_act, nb_steps,
                                                        reverse_z, need)
    gW, gb = _param_grads(dtheta if need[2] else None, W, b, nig[3], nig[4])
    return (dx if need[0] else None, dh if need[1] else None, None, gW, gb, None, None, None, None,
            glj if nig[9] else None)


flow_block.register_autograd(_flow_block_backward, setup_context=_flow_block_setup)


@torch.library.custom_op("umnn::flow_block_backward", mutates_args=(), device_types="cuda")
def flow_block_backward(x: Tensor, h: Tensor, scaling: Tensor, fx: Tensor, gz: Tensor, glj: Tensor, W: List[Tensor],
                        b: List[Tensor], hidden_act: int, out_act: int, nb_steps: int, reverse_z: bool,
                        need: List[bool]) -> tuple[Tensor, Tensor, Tensor]:
    """``FlowBlockTransform.backward`` without the z_2 hand-off (``integral.flow_block_vjp``)."""
    _check_flow_block_backward(x, h, scaling, fx, gz, glj, W, b, hidden_act, out_act, nb_steps, reverse_z, need)
    out = _I.flow_block_vjp(spec_from_tensors(W, b, hidden_act, out_act), pure_mlp(W, b, hidden_act, out_act), x, h, fx.contiguous(),
                            scaling.contiguous(), gz.contiguous(), glj.contiguous(), nb_steps, reverse_z, [bool(n) for n in need])
    like = (x, h, W[0])
    return tuple(t.contiguous() if n else _empty(l, torch.float32 if i == 2 else None)
                 for i, (t, n, l) in enumerate(zip(out, need, like)))


@flow_block_backward.register_fake
def _(x, h, scaling, fx, gz, glj, W, b, hidden_act, out_act, nb_steps, reverse_z, need):
    _check_flow_block_backward(x, h, scaling, fx, gz, glj, W, b, hidden_act, out_act, nb_steps, reverse_z, need)
    return (x.new_empty(x.shape) if need[0] else _empty(x), h.new_empty(h.shape) if need[1] else _empty(h),
            W[0].new_empty((_n_params(W, b),), dtype=torch.float32) if need[2] else _empty(W[0], torch.float32))


# ---------------------------------------------------------------------------------------------------------- log-likelihood
@torch.library.custom_op("umnn::flow_ll", mutates_args=(), device_types="cuda")
def flow_ll(z: Tensor, log_jac: Tensor) -> Tensor:
    """ll[b] = sum_i log_jac[b,i] - 1/2 sum_i (log 2 pi + z[b,i]^2): ``FlowLogLikelihood``'s launch (fp32 z and log_jac)."""
    _check_flow_ll(z, log_jac)
    return _I.hip_flow_ll(z, log_jac)


@flow_ll.register_fake
def _(z, log_jac):
    _check_flow_ll(z, log_jac)
    return z.new_empty((z.shape[0],), dtype=torch.float32)


@torch.library.custom_op("umnn::flow_ll_backward", mutates_args=(), device_types="cuda")
def flow_ll_backward(z: Tensor, g_ll: Tensor) -> tuple[Tensor, Tensor]:
    _check_flow_ll_backward(z, g_ll)
    return _I.hip_flow_ll_backward(z.contiguous(), g_ll, True, True)


@flow_ll_backward.register_fake
def _(z, g_ll):
    _check_flow_ll_backward(z, g_ll)
    return z.new_empty(z.shape), z.new_empty(z.shape)


def _flow_ll_setup(ctx, inputs, output):
    ctx.save_for_backward(inputs[0])


def _flow_ll_backward(ctx, g_ll):
    (z,) = ctx.saved_tensors
    gz, glj = torch.ops.umnn.flow_ll_backward(z, g_ll)
    return (gz if ctx.needs_input_grad[0] else None, glj if ctx.needs_input_grad[1] else None)


flow_ll.register_autograd(_flow_ll_backward, setup_context=_flow_ll_setup)


@torch.library.custom_op("umnn::flow_ll_block", mutates_args=(), device_types="cuda")
def flow_ll_block(x: Tensor, h: Tensor, scaling: Tensor, W: List[Tensor], b: List[Tensor], hidden_act: int, out_act: int,
                  nb_steps: int, reverse_z: bool, first: bool, last: bool, ll_in: Optional[Tensor]) -> tuple[Tensor, Tensor]:
    """One link of the one-pass log-likelihood (``hip_flow_ll_block``, inference): -> (z, ll); ``ll_in`` the running ll of the
    previous links (None for the first).  The [B,d] scratch is the op's own; the row counters are the shared zeroed buffer of
    the current stream (``integral.ll_counters``, which every launch leaves zero)."""
    _check_flow_ll_block(x, h, scaling, W, b, hidden_act, out_act, nb_steps, reverse_z, first, last, ll_in)
    x = x.contiguous()
    ll = torch.empty(x.shape[0], device=x.device, dtype=torch.float32) if ll_in is None else ll_in.clone()
    z = _I.hip_flow_ll_block(spec_from_tensors(W, b, hidden_act, out_act), x, h.contiguous(), scaling.contiguous(), nb_steps,
                             reverse_z, first, last, ll, torch.empty_like(x))
    return z, ll


@flow_ll_block.register_fake
def _(x, h, scaling, W, b, hidden_act, out_act, nb_steps, reverse_z, first, last, ll_in):
    _check_flow_ll_block(x, h, scaling, W, b, hidden_act, out_act, nb_steps, reverse_z, first, last, ll_in)
    return x.new_empty(x.shape), x.new_empty((x.shape[0],), dtype=torch.float32)


OPS = ("cc_forward", "cc_backward", "cc_forward_multi", "cc_forward_multi_nodes", "cc_cumulate", "cc_cumulate_adjoint", "cc_backward_multi_nodes", "cc_backward_multi", "cc_backward_multi_fx", "cc_solve", "cc_solve_block", "flow_block", "flow_block_backward", "flow_ll", "flow_ll_backward", "flow_ll_block")


spec_args = _I.spec_args       # MlpSpec -> (W[], b[], hidden_act, out_act): the integrand as the ops take it
