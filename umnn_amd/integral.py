"""The quadrature operator: ``integrate``, ``ParallelNeuralIntegral`` and ``NeuralIntegral``.

Same names, argument order and gradient convention as the reference
(models/UMNN/ParallelNeuralIntegral.py:37-123, models/UMNN/NeuralIntegral.py:37-99):

    ParallelNeuralIntegral.apply(x0, x, integrand, flat_params, h, nb_steps=20, inv_f=False)
    NeuralIntegral.apply(x0, x, integrand, flat_params, h, nb_steps=20)
    integrate(x0, nb_steps, step_sizes, integrand, h, compute_grad=False, x_tot=None, inv_f=False, ...)

backward returns (-f(x0;h)*g, f(x;h)*g, None, d_theta, d_h, None[, None]) -- the Leibniz derivatives for the
limits and the VJP of the integrand over the nodes for theta and h, exactly the reference's formulas.

Two execution paths, chosen per call, never silently:
  * HIP: the integrand is an MLP ``nets.mlp_spec`` recognises and the tensors live on a GPU.  One fused gfx950
    kernel per direction through the C ABI (include/umnn_cc.h).  If libumnn_cc.so is missing this raises.
    Both solvers ("CC" sequential, "CCParallel" materialised) are the same arithmetic, so both classes land on the
    same kernels; the node axis is never materialised.
  * generic ATen: arbitrary callables (lambdas, custom modules -- reference tests/test_numerical_validation.py:33-41,
    UMNNMAF.invert :207) cannot be compiled; they are integrated with torch ops on whatever device they live on,
    in node chunks so memory stays bounded.  MLP integrands on host tensors also take this path (the kernels
    need device memory); ``path_taken()`` reports which path the last call used so tests can assert on it.
"""
import ctypes
import math
import os
import weakref
import threading
import warnings

import torch
from torch.autograd.function import once_differentiable

from . import _lib
from ._common import _graph_mode, _ptr, _stream, traced_native_call  # noqa: F401  (the names are part of this module)
from .nets import graph_spec, mlp_spec, n_out_of, require_single
from .quadrature import compute_cc_weights, device_cumulative_adjoint, device_cumulative_matrix, device_tables

_state = threading.local()           # per-thread: last path taken, force_generic nesting
_warned = set()                       # fallbacks announced once per process (see _warn_once)


def _warn_once(key, message):
    """Every fallback off the HIP kernels is announced the first time it is taken (and ``path_taken()`` reports it)."""
    if key not in _warned:
        _warned.add(key)
        warnings.warn(message, RuntimeWarning, stacklevel=3)


_last_backward = {"path": None}      # process-wide: backward runs on autograd's worker threads, not on the caller's


def path_taken():
    """'hip' or 'aten': which path the calling thread's most recent forward (or directly called backward helper) used."""
    return getattr(_state, "path", None)


def backward_path_taken():
    """'hip' or 'aten': the path of the most recent quadrature BACKWARD in this process.  (autograd runs backward on its own
    worker threads, so the thread-local ``path_taken()`` of the caller does not see it.)"""
    return _last_backward["path"]


class force_generic:
    """Context manager: integrate MLP integrands with the generic ATen path too (A/B comparisons).  Thread-local: only the
    calling thread's integrals are rerouted (autograd's backward worker threads are told through the saved context)."""

    def __enter__(self):
        self._old = getattr(_state, "force_generic", False)
        _state.force_generic = True

    def __exit__(self, *exc):
        _state.force_generic = self._old


def _flatten(sequence):
    flat = [p.contiguous().view(-1) for p in sequence]
    return torch.cat(flat) if len(flat) > 0 else torch.tensor([])


# ----------------------------------------------------------------------------------------------
# HIP path
# ----------------------------------------------------------------------------------------------
_desc_cache = {}      # id(spec.linears[0]) -> (key, MlpDesc, keep-alive tensors)


def _desc(spec):
    """struct umnn_mlp for the current weights.  The weights are read live (optimizer steps / force_lipschitz write in
    place and are seen through the same pointers); the ctypes struct itself is rebuilt only when a pointer moved."""
    lins = spec.linears
    # (out_features too: row 0 of a multi-output last layer -- monotonic.OutputRow -- starts at the pointer of the whole matrix)
    key = tuple((lin.weight.data_ptr(), lin.bias.data_ptr(), lin.out_features) for lin in lins) + (spec.hidden_act, spec.out_act)
    slot = id(lins[0])
    hit = _desc_cache.get(slot)
    if hit is not None and hit[0] == key and hit[3] is lins[0]:
        return hit[1], hit[2]
    d = _lib.MlpDesc()
    d.n_linear = len(lins)
    d.widths[0] = lins[0].in_features
    keep = []
    cacheable = isinstance(lins[0], torch.nn.Module)     # (specs built from bare tensors, ops.py: rebuilt per call)
    for l, lin in enumerate(lins):
        w, b = lin.weight.detach(), lin.bias.detach()
        if not w.is_contiguous():
            w, cacheable = w.contiguous(), False       # a copy: its contents would go stale
        if not b.is_contiguous():
            b, cacheable = b.contiguous(), False
        keep += [w, b]
        d.widths[l + 1] = lin.out_features
        d.W[l], d.b[l] = w.data_ptr(), b.data_ptr()
    d.hidden_act, d.out_act = spec.hidden_act, spec.out_act
    if cacheable:
        if len(_desc_cache) > 256:
            _desc_cache.clear()
        _desc_cache[slot] = (key, d, keep, lins[0])
    return d, keep


def _use_hip(spec, x, graph=False):
    """The HIP kernels take this call.  ``graph`` (a call torch.compile / export / jit.trace records): the same rule without the
    thread-local ``force_generic`` switch and the one-time host warning, which traced code can neither read nor raise."""
    if spec is None or (not graph and getattr(_state, "force_generic", False)):
        return False
    if not x.is_cuda:
        if not graph:
            _warn_once("host", "umnn_amd: MLP integrand on host tensors -> generic ATen quadrature "
                               "(the HIP kernels need GPU tensors; move the model and data to 'cuda').")
        return False
    if x.dtype not in (torch.float32, torch.bfloat16, torch.float16):
        return False
    if spec.linears[0].weight.device != x.device:
        raise RuntimeError("umnn_amd: integrand weights and inputs are on different devices")
    return True


def _hip_spec(integrand, x, graph=None, multi=False, who="this operator"):
    """The MlpSpec of ``integrand`` when the HIP kernels take this call, else None: THE path decision, eager and recorded (there
    from ``nets.graph_spec``, which writes no cache onto the module).  ``graph``: ``_graph_mode()``, for callers that ask per block.
    ``multi``: the caller integrates a multi-output spec (the quadrature operators); every other caller refuses one, by name
    (``nets.require_single``), on every device.  Multi-output is defined for x [B,1] only: anything else raises here, on every path."""
    graph = _graph_mode() if graph is None else graph
    spec = graph_spec(integrand) if graph else mlp_spec(integrand)
    if not multi:
        require_single(spec, who)
    elif spec is not None and n_out_of(spec) > 1:
        _check_multi_x(n_out_of(spec), x)
    if not _use_hip(spec, x, graph):
        return None
    if n_out_of(spec) > 1 and not graph and not _multi_kernels_ok(spec):
        return None                      # (recorded calls: the ops make this choice when they run)
    return spec


def _check_multi_x(n_out, x):
    if x.dim() != 2 or x.shape[1] != 1:
        raise RuntimeError(f"umnn_amd: a multi-output integrand (n_out = {n_out}) is integrated over x of shape [B, 1]; got "
                           f"{tuple(x.shape)}.  Integrate the dimensions one by one, or use n_out = 1.")


def _kernel_probe(cache, key, spec, ask, warn_key, message):
    """Does the library have a kernel for this net: ``ask(desc)`` once per ``key`` (the widths, and whatever else decides) into
    ``cache``; a negative answer is announced once (``message(widths)``), and the caller runs on ATen.  -> the cached answer."""
    answer = cache.get(key)
    if answer is None:
        desc, keep = _desc(spec)
        answer = cache[key] = ask(ctypes.byref(desc))
    if answer < 0:
        widths = [m.out_features for m in spec.linears]
        _warn_once((warn_key, tuple((m.in_features, m.out_features) for m in spec.linears)), message(widths))
    return answer


_multi_ok = {}


def _multi_kernels_ok(spec):
    """False (after a one-time notice) for multi-output nets whose weight images, output image and scratch exceed the LDS: the
    library answers UMNN_EUNSUPPORTED and the quadrature runs on ATen, like the deep wide single-output nets' backward."""
    key = tuple((m.in_features, m.out_features) for m in spec.linears)
    return _kernel_probe(
        _multi_ok, key, spec, lambda desc: min(int(_lib.lib().umnn_cc_backward_multi_workspace_bytes(desc, 1, 1, key[0][0] - 1)), 0),
        "multi-aten", lambda widths: f"umnn_amd: no multi-output HIP kernel for integrand widths {widths} "
        f"({_lib.lib().umnn_last_error().decode('utf-8', 'replace')}): integrating with the generic ATen quadrature on the GPU.") >= 0


_bwd_kind = {}
_BWD_WIDE = {"hip": os.environ.get("UMNN_BWD_WIDE", "") == "hip"}     # read once; set_backward_wide() at run time


def set_backward_wide(force_hip):
    """True: nets whose HIP backward only has the register-spilling generic wide kernels use them anyway (default: the
    materialised ATen chain on the GPU; environment UMNN_BWD_WIDE=hip at import)."""
    _BWD_WIDE["hip"] = bool(force_hip)


def _hip_backward_ok(spec, x, h):
    """False for nets the HIP backward only covers with its register-spilling generic wide variants: since round 3 only deep
    nets whose zero-padded weight images exceed the LDS (four or more hidden layers above 103 units, five above 63) --
    unequal widths up to 127 otherwise run the shape-exact fp32 kernels zero-padded (cc_backward.hip pad_to_exact_family),
    and a wide FIRST hidden layer over a narrow rest (MNISTExperiment's 100-50-50-50-50) has the three-stage kernels of
    cc_backward_front.hip (both backward precisions since round 4).  ``UMNN_BWD_WIDE=hip`` forces the HIP kernels anyway."""
    if _BWD_WIDE["hip"]:
        return True
    E = h.shape[1] // x.shape[1]
    key = (tuple((m.in_features, m.out_features) for m in spec.linears), E, _lib.get_option("bwd_precision"))

    def ask(desc):
        kind = _lib.lib().umnn_cc_backward_kind(desc, E)
        if kind < -1:       # an error code (invalid descriptor, umnn_prepare_mlp failure): surfaced, never rerouted as "a wide net"
            _lib.check(kind, "umnn_cc_backward_kind")
        return kind

    return _kernel_probe(
        _bwd_kind, key, spec, ask, "bwd-aten",
        lambda widths: f"umnn_amd: the HIP backward has no shape-exact kernel for integrand widths {widths} "
        "(deep net of unequal wide hidden layers: its zero-padded weight images exceed the LDS): differentiating with the materialised ATen chain on the "
        "GPU instead (forward stays on the HIP kernel; umnn_amd.set_backward_wide(True) forces the HIP kernels).") >= 0


def _shape(spec, x, h):
    if x.dim() != 2 or h.dim() != 2 or h.shape[0] != x.shape[0]:
        raise RuntimeError("umnn_amd: expected x [B,d] and h [B,E*d]")
    B, d = x.shape
    E = h.shape[1] // d
    if E * d != h.shape[1] or spec.linears[0].in_features != 1 + E:
        raise RuntimeError(f"umnn_amd: h has {h.shape[1]} columns; the integrand expects (in_features-1)*d = "
                           f"{(spec.linears[0].in_features - 1) * d}")
    return B, d, E


def _f32c(t):
    return t.detach().to(torch.float32).contiguous()


def _io_prep(x_like, h):
    """Storage plan of one call (configuration C4: bf16 activations): tensors are handed to the kernels in the dtype the
    caller stores them in when that is fp32 or bf16 (no conversion pass, bf16 loads/stores inside the kernels); fp16 and
    anything else is converted to fp32 at the boundary.  -> (x dtype, h dtype, umnn_io pointer; None = all fp32: every ``_io``
    entry point takes a null descriptor for that)."""
    xd = x_like.dtype if x_like.dtype in (torch.float32, torch.bfloat16) else torch.float32
    hd = h.dtype if h.dtype in (torch.float32, torch.bfloat16) else torch.float32
    if xd == torch.float32 and hd == torch.float32:
        return xd, hd, None
    io = _lib.IoDesc(_lib.DTYPE_BF16 if xd == torch.bfloat16 else _lib.DTYPE_F32,
                     _lib.DTYPE_BF16 if hd == torch.bfloat16 else _lib.DTYPE_F32)
    return xd, hd, ctypes.byref(io)


def _as(t, dtype):
    return None if t is None else t.detach().to(dtype).contiguous()


def _quad_plan(spec, x, h, multi):
    """Shape check and storage plan of the four quadrature wrappers -> (B, d, E, x storage dtype, h storage dtype, umnn_io pointer).
    ``multi``: the multi-output entries are exact fp32 whatever ``set_precision`` says and take no descriptor: bf16 / fp16 callers
    are converted at the boundary."""
    if multi:
        _check_multi_x(n_out_of(spec), x)
    return _shape(spec, x, h) + ((torch.float32, torch.float32, None) if multi else _io_prep(x, h))


def _quad_done(rc, fn_name, x_outs, stored, x_dtype, backward=False):
    """What the four end with: ``check``, the path bookkeeping, and the x-shaped outputs from their ``stored`` dtype back to the
    caller's (fp16 callers, bf16 ones of the multi-output entries: fp32 inside, theirs outside)."""
    _lib.check(rc, fn_name)
    _state.path = "hip"
    if backward:
        _last_backward["path"] = "hip"
    if x_dtype == stored:
        return x_outs
    return tuple(None if t is None else t.to(x_dtype) for t in x_outs)


def hip_forward(spec, x0, x, h, nb_steps, inv_f=False, multi=False):
    """-> (F, f_x, f_x0), each [B,d] in x's dtype.  x0 may be None (zeros).  ``multi``: the body of ``hip_forward_multi``."""
    lib = _lib.lib()
    B, d, E, xd, hd, io = _quad_plan(spec, x, h, multi)
    out_dtype = x.dtype
    x, h, x0 = _as(x, xd), _as(h, hd), _as(x0, xd)
    w, s = device_tables(nb_steps, x.device)
    shape = (B, n_out_of(spec) if multi else d)
    F, fx, fx0 = x.new_empty(shape), x.new_empty(shape), x.new_empty(shape)
    desc, keep = _desc(spec)
    with torch.cuda.device(x.device):
        tail = (_ptr(x0), _ptr(x), _ptr(h), _ptr(w), _ptr(s), int(nb_steps), B, d, E, int(bool(inv_f)), _ptr(F), _ptr(fx), _ptr(fx0),
                _stream(x.device))
        rc = lib.umnn_cc_forward_multi(ctypes.byref(desc), *tail) if multi else lib.umnn_cc_forward_io(ctypes.byref(desc), io, *tail)
    return _quad_done(rc, "umnn_cc_forward_multi" if multi else "umnn_cc_forward", (F, fx, fx0), xd, out_dtype)


def hip_forward_multi(spec, x0, x, h, nb_steps, inv_f=False):
    """Multi-output forward (umnn_cc_forward_multi): x [B,1], h [B,E] -> (F, f_x, f_x0), each [B, n_out] in x's dtype.  Exact fp32
    kernels and fp32 storage whatever ``set_precision`` says; bf16 / fp16 callers are converted at the boundary."""
    return hip_forward(spec, x0, x, h, nb_steps, inv_f, multi=True)


def hip_forward_multi_nodes(spec, x0, x, h, nb_steps):
    """The forward that keeps its nodes (umnn_cc_forward_multi_nodes): x [B,1], h [B,E], n_out = 1..16 -> (F [B, n_out],
    f_nodes [B, nb_steps + 1, n_out]) in x's dtype, f_nodes[:, j] = f(t_j; h) in NODE order (node 0 is x, node n is x0).  Exact fp32
    like every multi-output entry."""
    B, d, E, xd, hd, io = _quad_plan(spec, x, h, True)
    out_dtype, K = x.dtype, n_out_of(spec)
    x, h, x0 = _as(x, xd), _as(h, hd), _as(x0, xd)
    w, s = device_tables(nb_steps, x.device)
    F, f_nodes = x.new_empty((B, K)), x.new_empty((B, int(nb_steps) + 1, K))
    desc, keep = _desc(spec)
    with torch.cuda.device(x.device):
        rc = _lib.lib().umnn_cc_forward_multi_nodes(ctypes.byref(desc), _ptr(x0), _ptr(x), _ptr(h), _ptr(w), _ptr(s), int(nb_steps),
                                                    B, d, E, _ptr(F), _ptr(f_nodes), _stream(x.device))
    return _quad_done(rc, "umnn_cc_forward_multi_nodes", (F, f_nodes), xd, out_dtype)


def hip_cumulate(values, x0, x, nb_steps, ascending=False):
    """umnn_cc_cumulate: values [B, nb_steps + 1, K] at the nodes of [x0, x] (x, x0 [B,1]; x0 None: zeros), K <= 16 -> the integral from
    x0 up to every node, [B, nb_steps + 1, K] in values' dtype, ASCENDING from the lower limit (index 0, exactly 0) to x.  ``values``
    in node order (what ``hip_forward_multi_nodes`` leaves), or -- ``ascending`` -- from the lower limit up, like the result.  It has
    no integrand, hence no ``_quad_plan``; it ends like the other wrappers, in ``_quad_done``."""
    n = int(nb_steps)
    _check_cumulate(values, x0, x, n)
    B, K = values.shape[0], values.shape[2]
    out_dtype = values.dtype
    values, x, x0 = _as(values, torch.float32), _as(x, torch.float32), _as(x0, torch.float32)
    Q = device_cumulative_matrix(n, values.device, ascending)
    out = torch.empty_like(values)
    with torch.cuda.device(values.device):
        rc = _lib.lib().umnn_cc_cumulate(_ptr(Q), _ptr(values), _ptr(x0), _ptr(x), n, B, K, _ptr(out), _stream(values.device))
    return _quad_done(rc, "umnn_cc_cumulate", (out,), torch.float32, out_dtype)[0]


def hip_cumulate_adjoint(g, nb_steps, ascending=False):
    """umnn_cc_cumulate_adjoint: g [B, nb_steps + 1, K], the cotangent of ``hip_cumulate``'s (ascending) output -> sum_i Qt[j, i] g[:, i],
    [B, nb_steps + 1, K] in g's dtype: the cotangent of that call's ``values`` up to the factor (x - x0)/2, which the caller applies --
    in node order, or -- ``ascending`` -- from the lower limit up, like the values were."""
    n = int(nb_steps)
    if g.dim() != 3 or g.shape[1] != n + 1:
        raise RuntimeError(f"umnn_amd: the cotangent of a cumulative quadrature is [B, nb_steps + 1, K]; got {tuple(g.shape)} at nb_steps = {n}")
    out_dtype = g.dtype
    g = _as(g, torch.float32)
    Qt = device_cumulative_adjoint(n, g.device, ascending)
    out = torch.empty_like(g)
    with torch.cuda.device(g.device):
        rc = _lib.lib().umnn_cc_cumulate_adjoint(_ptr(Qt), _ptr(g), n, g.shape[0], g.shape[2], _ptr(out), _stream(g.device))
    return _quad_done(rc, "umnn_cc_cumulate_adjoint", (out,), torch.float32, out_dtype, backward=True)[0]


def hip_backward_multi_nodes(spec, x0, x, h, cot_nodes, nb_steps, need=(True, True, True, True)):
    """umnn_cc_backward_multi_nodes: the multi-output backward for a cotangent PER NODE, cot_nodes [B, nb_steps + 1, n_out] of
    f_k(t_j; h) in node order (node 0 is x), n_out = 1..16 -> (dx0_tau, dx_tau, dh, dtheta_flat), None where ``need`` is False:
    dh / dtheta = sum_j VJP_f(t_j, h)[cot_nodes[:, j]], dx_tau = sum_j (u_j / 2) tau_j and dx0_tau = sum_j (1 - u_j / 2) tau_j with
    tau_j = sum_k cot_nodes[:, j, k] df_k/dt (t_j), u = s + 1 -- what the limits do through the nodes; no weight, no span factor
    and no Leibniz term (``aten_vjp_nodes`` is the same on ATen).  Exact fp32 like every multi-output entry."""
    lib = _lib.lib()
    B, d, E, xd, hd, io = _quad_plan(spec, x, h, True)
    K, n = n_out_of(spec), int(nb_steps)
    if cot_nodes.shape != (B, n + 1, K):
        raise RuntimeError(f"umnn_amd: the node cotangents have shape {tuple(cot_nodes.shape)}; expected {(B, n + 1, K)}")
    x_dtype, h_dtype = x.dtype, h.dtype
    x, h, x0, cot = _as(x, xd), _as(h, hd), _as(x0, xd), _as(cot_nodes, xd)
    _, s = device_tables(n, x.device)
    dx0 = torch.empty_like(x) if need[0] else None
    dx = torch.empty_like(x) if need[1] else None
    dh = torch.empty_like(h) if need[2] else None
    n_params = sum(l.weight.numel() + l.bias.numel() for l in spec.linears)
    dtheta = torch.empty(n_params, device=x.device, dtype=torch.float32) if need[3] else None
    desc, keep = _desc(spec)
    net = ctypes.byref(desc)
    with torch.cuda.device(x.device):
        nbytes = int(lib.umnn_cc_backward_multi_nodes_workspace_bytes(net, B, E))
        if nbytes < 0:
            _lib.check(_lib.EUNSUPPORTED, "umnn_cc_backward_multi_nodes_workspace_bytes")
        ws = torch.empty(max(nbytes, 4), device=x.device, dtype=torch.uint8)
        rc = lib.umnn_cc_backward_multi_nodes(net, _ptr(x0), _ptr(x), _ptr(h), _ptr(cot), _ptr(s), n, B, 1, E, _ptr(dx0), _ptr(dx),
                                              _ptr(dh), _ptr(dtheta), _ptr(ws), nbytes, _stream(x.device))
    dx0, dx = _quad_done(rc, "umnn_cc_backward_multi_nodes", (dx0, dx), xd, x_dtype, backward=True)
    if h_dtype != hd and dh is not None:
        dh = dh.to(h_dtype)
    return dx0, dx, dh, dtheta


_curve_ok = {}
_curve_grad_ok = {}


def _curve_grad_kernels_ok(spec, nb_steps):
    """``_curve_kernels_ok`` and the same question for the two entries of the curve's backward, asked with zero rows: False (after a
    one-time notice) sends a curve that is differentiated to ``aten_curve`` under autograd."""
    if not _curve_kernels_ok(spec, nb_steps):
        return False
    key = (tuple((m.in_features, m.out_features) for m in spec.linears), int(nb_steps))

    def ask(desc):
        lib = _lib.lib()
        for name, rc in (("umnn_cc_backward_multi_nodes", lib.umnn_cc_backward_multi_nodes(
                              desc, None, None, None, None, None, key[1], 0, 1, key[0][0][0] - 1, None, None, None, None, None, 0, None)),
                         ("umnn_cc_cumulate_adjoint", lib.umnn_cc_cumulate_adjoint(None, None, key[1], 0, key[0][-1][1], None, None))):
            if rc == _lib.EUNSUPPORTED:
                return rc
            _lib.check(rc, name)
        return 0

    return _kernel_probe(
        _curve_grad_ok, key, spec, ask, "curve-grad-aten", lambda widths: f"umnn_amd: no HIP curve backward for integrand widths {widths} "
        f"at nb_steps = {key[1]} ({_lib.lib().umnn_last_error().decode('utf-8', 'replace')}): the curve runs on the generic ATen path "
        "under autograd.") >= 0


def _curve_kernels_ok(spec, nb_steps):
    """False (after a one-time notice) when the library answers UMNN_EUNSUPPORTED for a curve of this net and nb_steps -- weight images
    beyond the LDS, or a cumulative table beyond its LDS budget (nb_steps > 127): asked with zero rows, which launches nothing."""
    key = (tuple((m.in_features, m.out_features) for m in spec.linears), int(nb_steps))

    def ask(desc):
        lib = _lib.lib()
        for name, rc in (("umnn_cc_forward_multi_nodes", lib.umnn_cc_forward_multi_nodes(desc, None, None, None, None, None, key[1], 0, 1,
                                                                                        key[0][0][0] - 1, None, None, None)),
                         ("umnn_cc_cumulate", lib.umnn_cc_cumulate(None, None, None, None, key[1], 0, key[0][-1][1], None, None))):
            if rc == _lib.EUNSUPPORTED:
                return rc
            _lib.check(rc, name)
        return 0

    return _kernel_probe(
        _curve_ok, key, spec, ask, "curve-aten", lambda widths: f"umnn_amd: no HIP curve kernels for integrand widths {widths} at "
        f"nb_steps = {key[1]} ({_lib.lib().umnn_last_error().decode('utf-8', 'replace')}): the curve runs on the generic ATen path.") >= 0


def _add_h0(dh, h0_cot, d):
    """d_h + the h_0 term in embedding row 0 (z carries h_0 = embedding row 0, UMNNMAF.py:80), in fp32, in dh's dtype"""
    out = dh.float() if dh.dtype != torch.float32 else dh
    out.view(dh.shape[0], -1, d)[:, 0, :].add_(h0_cot)
    return out.to(dh.dtype)


def hip_backward(spec, x0, x, h, g, g_fx, nb_steps, need=(True, True, True, True), inv_f=False, z2_saved=None, h0_cot=None, multi=False):
    """-> (dx0, dx, dh, dtheta_flat); entries are None where need[...] is False.  dx0/dx come back in x's dtype, dh in
    h's, dtheta in fp32 (the weights' dtype).  inv_f: the operator integrated 1/f (ParallelNeuralIntegral.py:58-59,70-72).
    h0_cot [B,d] (a flow block's backward: lower limit 0): added to embedding row 0 of dh by the kernel that stores dh
    (umnn_cc_backward_block_io, the entry of every call without x0, inv_f and d_x0; ``z2_saved`` is that entry's too), so that a
    bf16 dh is rounded once.  ``multi``: the body of ``hip_backward_multi``."""
    lib = _lib.lib()
    B, d, E, xd, hd, io = _quad_plan(spec, x, h, multi)
    if multi:
        K = n_out_of(spec)
        if g.shape != (B, K):
            raise RuntimeError(f"umnn_amd: the cotangent of a multi-output integral has shape {tuple(g.shape)}; expected {(B, K)}")
        if g_fx is not None and g_fx.shape != (B, K):
            raise RuntimeError(f"umnn_amd: the cotangent of the f_x output of a multi-output integral has shape {tuple(g_fx.shape)}; expected {(B, K)}")
    x_dtype, h_dtype = x.dtype, h.dtype
    x, h, g, x0, g_fx = _as(x, xd), _as(h, hd), _as(g, xd), _as(x0, xd), _as(g_fx, xd)
    w, s = device_tables(nb_steps, x.device)
    dx0 = torch.empty_like(x) if need[0] else None
    dx = torch.empty_like(x) if need[1] else None
    dh = torch.empty_like(h) if need[2] else None
    n_params = sum(l.weight.numel() + l.bias.numel() for l in spec.linears)
    dtheta = torch.empty(n_params, device=x.device, dtype=torch.float32) if need[3] else None
    desc, keep = _desc(spec)
    net = ctypes.byref(desc)
    with torch.cuda.device(x.device):
        nbytes = (lib.umnn_cc_backward_multi_workspace_bytes if multi else lib.umnn_cc_backward_workspace_bytes)(net, B, d, E)
        if multi and nbytes < 0:
            _lib.check(_lib.EUNSUPPORTED, "umnn_cc_backward_multi_workspace_bytes")
        ws = torch.empty(max(int(nbytes), 4), device=x.device, dtype=torch.uint8)
        mid = (_ptr(x), _ptr(h), _ptr(g), _ptr(g_fx), _ptr(w), _ptr(s), int(nb_steps), B, d, E)
        outs = (_ptr(dx), _ptr(dh), _ptr(dtheta))
        end = (_ptr(ws), int(nbytes), _stream(x.device))
        h0 = _as(h0_cot, torch.float32) if dh is not None else None
        if multi:
            rc = lib.umnn_cc_backward_multi_fx(net, _ptr(x0), *mid, int(bool(inv_f)), _ptr(dx0), *outs, *end)
        elif x0 is None and not inv_f and not need[0]:      # (the flow block's entry has no x0 and no d_x0 output; h0 and z_2 nullable)
            rc = lib.umnn_cc_backward_block_io(net, io, *mid, _ptr(h0), *outs, _ptr(z2_saved),
                                               0 if z2_saved is None else int(z2_saved.numel()), *end)
            h0 = None
        else:
            rc = lib.umnn_cc_backward_io(net, io, _ptr(x0), *mid, int(bool(inv_f)), _ptr(dx0), *outs, *end)
    dx0, dx = _quad_done(rc, "umnn_cc_backward_multi_fx" if multi else "umnn_cc_backward", (dx0, dx), xd, x_dtype, backward=True)
    if h0 is not None:
        dh = _add_h0(dh, h0, d)
    if h_dtype != hd and dh is not None:
        dh = dh.to(h_dtype)
    return dx0, dx, dh, dtheta


def hip_backward_multi(spec, x0, x, h, g, nb_steps, need=(True, True, True, True), inv_f=False, g_fx=None):
    """Multi-output backward (umnn_cc_backward_multi_fx) for the cotangent g [B, n_out] -> (dx0, dx, dh, dtheta_flat), None where
    ``need`` is False: dx = sum_k g_k f_k(x) and dx0 = -sum_k g_k f_k(x0) are [B,1]; dtheta is flat in parameters() order with
    the last layer as [n_out, H_L] / [n_out].  ``g_fx`` [B, n_out] (optional): the cotangent of the f_x output, f_k(x; h) -- it
    reaches dh and dtheta through the same launches and adds sum_k g_fx,k df_k/dx (x) to dx."""
    return hip_backward(spec, x0, x, h, g, g_fx, nb_steps, need, inv_f, multi=True)


# z_2 handed from the training forward to the backward (three-stage family): memory held from forward to backward.  Two caps: per
# block (UMNN_SAVE_Z2_MAX_GB, default 2) and over everything alive at once -- all blocks of a flow between its forward and its
# backward -- (UMNN_SAVE_Z2_TOTAL_GB, default 8; the 5-block MNISTExperiment flow at B = 100 holds 4.2 GB).  Above either, that block's
# backward recomputes z_2 (its stage A) as before: a speed / peak-memory trade, never a different result.
_Z2_MAX_BYTES = int(float(os.environ.get("UMNN_SAVE_Z2_MAX_GB", "2")) * (1 << 30))
_Z2_TOTAL_BYTES = int(float(os.environ.get("UMNN_SAVE_Z2_TOTAL_GB", "8")) * (1 << 30))
_z2_live = [0]


def _z2_release(nbytes):
    _z2_live[0] -= nbytes


def _z2_buffer(desc, x, h, B, d, E, nb_steps):
    """-> (z2, floats): the fp32 buffer umnn_cc_backward_saved wants, or (None, 0) when the pair does not apply to this net / storage /
    arithmetic mode or the buffer would exceed either cap."""
    # (fp32 x-class tensors; the embedding h in fp32 or -- configuration C4 -- bf16, loaded as such by the kernels)
    if x.dtype != torch.float32 or h.dtype not in (torch.float32, torch.bfloat16):
        return None, 0
    nfl = int(_lib.lib().umnn_cc_forward_z2_floats(ctypes.byref(desc), B, d, E, int(nb_steps)))
    if not (0 < 4 * nfl <= _Z2_MAX_BYTES and _z2_live[0] + 4 * nfl <= _Z2_TOTAL_BYTES):
        return None, 0
    z2 = torch.empty(nfl, device=x.device, dtype=torch.float32)
    _z2_live[0] += 4 * nfl
    weakref.finalize(z2, _z2_release, 4 * nfl)
    return z2, nfl


def hip_flow_block(spec, x, h, scaling, nb_steps, reverse_z=False, log_jac_in=None, save_z2=False):
    """Fused block epilogue -> (z, log_jac, f_x, f_x0).  ``reverse_z``: z comes back with its dimensions reversed (the
    flip between the blocks of a flow); ``log_jac_in``: running log_jac of the previous blocks, added in the kernel.
    ``save_z2`` (training forward): -> (z, log_jac, f_x, f_x0, z2) where z2 is the buffer umnn_cc_backward_saved wants, or None when
    the pair does not apply to this net / arithmetic mode or the buffer would exceed UMNN_SAVE_Z2_MAX_GB (default 2) per block."""
    lib = _lib.lib()
    B, d, E = _shape(spec, x, h)
    desc, keep = _desc(spec)
    z2, nfl = _z2_buffer(desc, x, h, B, d, E, nb_steps) if save_z2 else (None, 0)
    out_dtype = x.dtype
    xd, hd, io = _io_prep(x, h)
    x, h, scaling, lj_in = _as(x, xd), _as(h, hd), _f32c(scaling), _as(log_jac_in, xd)
    w, s = device_tables(nb_steps, x.device)
    z, lj, fx, fx0 = (torch.empty_like(x) for _ in range(4))
    args = (ctypes.byref(desc), io, _ptr(x), _ptr(h), _ptr(scaling), _ptr(w), _ptr(s), int(nb_steps), B, d, E, 1 if reverse_z else 0,
            _ptr(lj_in), _ptr(z), _ptr(lj), _ptr(fx), _ptr(fx0))
    with torch.cuda.device(x.device):
        rc = lib.umnn_flow_stack_block_forward_save_io(*args, _ptr(z2), nfl, _stream(x.device)) if z2 is not None else _lib.EUNSUPPORTED
        if rc == _lib.EUNSUPPORTED:         # no z_2 hand-off (not asked for, capped, or the library says it does not apply)
            z2 = None
            rc = lib.umnn_flow_stack_block_forward_io(*args, _stream(x.device))
    _lib.check(rc, "umnn_flow_stack_block_forward")
    _state.path = "hip"
    if out_dtype != xd:
        z, lj, fx, fx0 = z.to(out_dtype), lj.to(out_dtype), fx.to(out_dtype), fx0.to(out_dtype)
    return (z, lj, fx, fx0, z2) if save_z2 else (z, lj, fx, fx0)


def _inverse_call(fn_name, spec, h, rows, nb_steps, call, warn_key, warn_text):
    """What the in-kernel inverse entry points share: ``rows`` [B,d] gives B, d and the device; checks the embedding, makes the
    quadrature tables and runs ``call(lib, desc, w, s, B, d, E, stream)`` -> rc on the current stream.  False (after a one-time
    warning) when the library has no kernel for this net, else True; any other error raises."""
    lib = _lib.lib()
    B, d = rows.shape
    E = h.shape[1] // d
    if E * d != h.shape[1] or spec.linears[0].in_features != 1 + E:
        raise RuntimeError("umnn_amd: embedding width does not match the integrand")
    w, s = device_tables(nb_steps, rows.device)
    desc, keep = _desc(spec)
    with torch.cuda.device(rows.device):
        rc = call(lib, ctypes.byref(desc), _ptr(w), _ptr(s), B, d, E, _stream(rows.device))
    if rc == _lib.EUNSUPPORTED:
        _warn_once((warn_key, tuple(l.out_features for l in spec.linears), _lib.get_forward_precision()),
                   warn_text.format(_lib.lib().umnn_last_error().decode('utf-8', 'replace')))
        return False
    _lib.check(rc, fn_name)
    _state.path = "hip"
    return True


def hip_invert_dim(spec, h, z, scaling, nb_steps, j, iters, x_inv):
    """Bracket search of flow dimension j for every sample in ONE launch (umnn_flow_invert_dim): writes x_inv[:, j].
    Returns False when the library has no kernel for this net (single hidden layer / LDS): the caller keeps its own loop."""
    return _inverse_call(
        "umnn_flow_invert_dim", spec, h, z, nb_steps,
        lambda lib, desc, w, s, B, d, E, stream: lib.umnn_flow_invert_dim(
            desc, _ptr(h), _ptr(z), _ptr(scaling), w, s, int(nb_steps), B, d, E, int(j), int(iters), _ptr(x_inv), stream),
        "invert-host", "umnn_amd: no in-kernel inversion for this integrand / arithmetic mode ({}): UMNNMAF.invert runs the "
        "host-driven bracket search (d x iter forward launches per block).")


def _solve_call(fn_name, spec, h, target, nb_steps, x_out, want_info, info_shape, call, fx_shape=None):
    """hip_solve / hip_solve_block / hip_solve_multi: allocates x_out (when None) and the ``info_shape`` f_x / status (when
    ``want_info``; ``fx_shape``: an f_x of another shape than status, the [B,K] of the multi-output solve), runs
    ``call(lib, desc, w, s, B, d, E, stream, x_out, fx, status)`` -> rc.  -> (x_out, f_x, status), or None without a kernel."""
    dev = target.device
    if x_out is None:
        x_out = torch.empty(target.shape, device=dev, dtype=torch.float32)
    fx = torch.empty(info_shape if fx_shape is None else fx_shape, device=dev, dtype=torch.float32) if want_info else None
    status = torch.empty(info_shape, device=dev, dtype=torch.int32) if want_info else None
    ok = _inverse_call(
        fn_name, spec, h, target, nb_steps, lambda *a: call(*a, _ptr(x_out), _ptr(fx), _ptr(status)),
        "solve-host", "umnn_amd: no in-kernel Newton solve for this integrand / arithmetic mode ({}): the inverse runs the "
        "host-driven Newton loop (one forward launch per iteration).")
    if not ok:
        _state.host_solve = True        # (graphs.GraphedSampler: a host-driven Newton loop reads the device and cannot be captured)
    return (x_out, fx, status) if ok else None


def hip_solve(spec, h, target, nb_steps, j=0, scale_row=None, scaling=None, off_row=None, off_h0=False, lo=-50., hi=50., tol=1e-6,
              max_iter=64, x_out=None, want_info=True, lj_row=None, lj_first=False):
    """Newton solve of dimension j for every row in ONE launch (umnn_cc_solve), the counterpart of ``hip_invert_dim``:
    scale (off + int_0^x f(t; h[:, :, j]) dt) = target[:, j].  ``target`` [B,d] fp32 contiguous, ``h`` [B,E*d] fp32 contiguous;
    scale = ``scale_row`` [B], else exp(``scaling``[j]), else 1; off = ``off_row`` [B], else embedding row 0 (``off_h0``), else 0.
    Writes ``x_out``[:, j] ([B,d] fp32 contiguous; allocated when None) -> (x_out, f_x [B], status [B] int32), the last two None
    unless ``want_info``.  Returns None when the library has no kernel for this net: the caller runs ``host_solve``.
    ``lj_row`` [B] fp32 contiguous (umnn_cc_solve_lj, the same launch): gets log(f(x) + 1e-10) + s added in place -- s = ``scaling``[j],
    else log(``scale_row``), else 0 --, or written over whatever it holds when ``lj_first``."""
    if lj_row is None:
        return _solve_call(
            "umnn_cc_solve", spec, h, target, nb_steps, x_out, want_info, target.shape[:1],
            lambda lib, desc, w, s, B, d, E, stream, x, fx, status: lib.umnn_cc_solve(
                desc, _ptr(h), _ptr(target), d, _ptr(scale_row), _ptr(scaling), _ptr(off_row), 1 if off_h0 else 0, w, s, int(nb_steps),
                B, d, E, int(j), float(lo), float(hi), float(tol), int(max_iter), x, d, fx, status, stream))
    if lj_row.dtype != torch.float32 or not lj_row.is_contiguous() or lj_row.shape != target.shape[:1] or lj_row.device != target.device:
        raise ValueError("umnn_amd: hip_solve needs lj_row as a contiguous fp32 [B] tensor on the target's device")
    return _solve_call(
        "umnn_cc_solve_lj", spec, h, target, nb_steps, x_out, want_info, target.shape[:1],
        lambda lib, desc, w, s, B, d, E, stream, x, fx, status: lib.umnn_cc_solve_lj(
            desc, _ptr(h), _ptr(target), d, _ptr(scale_row), _ptr(scaling), _ptr(off_row), 1 if off_h0 else 0, w, s, int(nb_steps),
            B, d, E, int(j), float(lo), float(hi), float(tol), int(max_iter), x, d, fx, status, _ptr(lj_row), 1 if lj_first else 0, stream))


def hip_solve_block(spec, h, target, nb_steps, scaling=None, off_h0=False, x_init=None, lo=-50., hi=50., tol=1e-6, max_iter=64,
                    want_info=True, x_out=None):
    """Newton solve of EVERY (row, dimension) of a block under the given embedding in ONE launch (umnn_cc_solve_block):
    exp(scaling[i]) (off + int_0^x f(t; h[b, :, i]) dt) = target[b, i], off = h[b, 0*d + i] when ``off_h0``.  ``target`` [B,d] and ``h``
    [B,E*d] fp32 contiguous; ``x_init`` [B,d] fp32 contiguous or None: the first iterate of every row (clamped into [lo, hi]; a
    non-finite entry starts that row at 0; may be ``x_out`` itself).  -> (x [B,d], f_x [B,d], status [B,d] int32), the last two None
    unless ``want_info``.  Returns None when the library has no kernel for this net: the caller runs ``host_solve``."""
    return _solve_call(
        "umnn_cc_solve_block", spec, h, target, nb_steps, x_out, want_info, target.shape,
        lambda lib, desc, w, s, B, d, E, stream, x, fx, status: lib.umnn_cc_solve_block(
            desc, _ptr(h), _ptr(target), _ptr(scaling), 1 if off_h0 else 0, _ptr(x_init), w, s, int(nb_steps), B, d, E,
            float(lo), float(hi), float(tol), int(max_iter), x, fx, status, stream))


def hip_solve_multi(spec, h, target, coef, nb_steps, lo=-50., hi=50., tol=1e-6, max_iter=64):
    """Newton solve of a weighted sum of the K outputs of a multi-output integrand for every row in ONE launch
    (umnn_cc_solve_multi): sum_k coef[b,k] int_0^x f_k(t; h_b) dt = target[b].  ``target`` [B,1], ``coef`` [B,K] and ``h`` [B,E] fp32
    contiguous.  -> (x [B,1], F [B,K], f_x [B,K], status [B,1] int32), F_k and f_k at the returned x.  Exact fp32 kernels whatever
    ``set_precision`` says.  Returns None when the library has no kernel for this net (its images exceed the LDS): the caller runs
    ``newton_solve_sum`` over ``hip_forward_multi``."""
    B, K = target.shape[0], n_out_of(spec)
    if target.shape != (B, 1) or coef.shape != (B, K):
        raise RuntimeError(f"umnn_amd: the weighted-sum solve takes a target [B, 1] and coefficients [B, {K}]; got "
                           f"{tuple(target.shape)} and {tuple(coef.shape)}")
    F = torch.empty((B, K), device=target.device, dtype=torch.float32)
    out = _solve_call(
        "umnn_cc_solve_multi", spec, h, target, nb_steps, None, True, (B, 1),
        lambda lib, desc, w, s, B, d, E, stream, x, fx, status: lib.umnn_cc_solve_multi(
            desc, _ptr(h), _ptr(target), _ptr(coef), w, s, int(nb_steps), B, E, float(lo), float(hi), float(tol), int(max_iter),
            x, _ptr(F), fx, status, stream), fx_shape=(B, K))
    return None if out is None else (out[0], F, out[1], out[2])


def newton_solve(eval_fn, target, scale, off, lo, hi, tol, max_iter, x_init=None):
    """The safeguarded Newton iteration of umnn_cc_solve (include/umnn_cc.h) in torch ops, elementwise on tensors of any shape:
    solves scale (off + F(x)) = target on [lo, hi], where ``eval_fn(x) -> (F(x), f(x))`` with f = dF/dx > 0.  The host-driven
    loop over ``hip_forward`` and the generic ATen path are this function.  ``x_init`` (shaped like ``target``, optional): the first
    iterate, clamped into [lo, hi]; non-finite entries start at 0 like every row without it.  -> (x, f(x), status int32)."""
    lo, hi = float(lo), float(hi)
    x = torch.full_like(target, min(max(0., lo), hi))
    if x_init is not None:
        x = torch.where(torch.isfinite(x_init), x_init.to(target.dtype), torch.zeros_like(target)).clamp(lo, hi)
    a, b = torch.full_like(target, lo), torch.full_like(target, hi)
    a_open = torch.ones_like(target, dtype=torch.bool)
    b_open, done, bad = a_open.clone(), ~a_open, ~a_open
    evals = torch.zeros_like(target, dtype=torch.int32)
    flags = torch.zeros_like(evals)
    fx = torch.zeros_like(target)
    bound = tol * target.abs().clamp(min=1.)
    for it in range(int(max_iter)):
        F, f = eval_fn(x)
        act = ~done
        evals += act
        fx = torch.where(act, f, fx)
        r = scale * (off + F) - target
        nonfinite = act & (~torch.isfinite(F) | torch.isnan(r))
        bad |= nonfinite
        done = done | nonfinite | (act & (r.abs() <= bound) & torch.isfinite(r))    # (no x meets an infinite target: its bound is infinite too)
        act = ~done
        pos = r > 0
        clamped = act & ((pos & (x <= lo)) | (~pos & (x >= hi)))       # the target lies beyond G(lo) / G(hi)
        flags |= clamped.to(torch.int32) * _lib.SOLVE_CLAMPED
        b = torch.where(act & pos, x, b)
        a = torch.where(act & ~pos, x, a)
        b_open &= ~(act & pos)
        a_open &= ~(act & ~pos)
        done = done | clamped
        act = ~done
        xn = x - r / (scale * f)
        inside = (xn > a) & (xn < b)
        to_b = ~inside & (xn >= b) & b_open                           # overshot an endpoint not yet evaluated: try it
        to_a = ~inside & ~to_b & (xn <= a) & a_open
        use_mid = ~inside & ~to_b & ~to_a
        mid = 0.5 * (a + b)
        collapsed = use_mid & ~((mid > a) & (mid < b))                # adjacent floats
        xn = torch.where(to_b, b, torch.where(to_a, a, torch.where(use_mid, mid, xn)))
        b_open &= ~(act & to_b)
        a_open &= ~(act & to_a)
        done = done | (act & collapsed)
        done = done | (~done & (xn == x))                             # x has stopped changing
        if bool(done.all()):
            break
        if it + 1 < max_iter:
            x = torch.where(done, x, xn)                              # (the last evaluated point is what leaves)
    flags |= (~done).to(torch.int32) * _lib.SOLVE_CAPPED
    flags |= bad.to(torch.int32) * _lib.SOLVE_NONFINITE
    x = torch.where(bad, torch.full_like(x, float("nan")), x)
    return x, fx, evals | flags


def quadrature_eval(spec, integrand, h, nb_steps, use_hip, column=False):
    """``eval_fn(x) -> (F(x), f(x))`` for ``newton_solve``, F = int_0^x f(t; h) dt, whenever the iteration is driven from the host:
    ``use_hip`` one ``hip_forward`` launch per call (F and f_x together), else the ATen quadrature and one pass of the integrand.
    ``h`` is used as given (the caller brings it to x's dtype for the ATen form).  ``column``: x is the [B,1] column of one flow
    dimension and ``h`` its [B,E] embedding rows, which the ATen form evaluates through ``integrand.independant_forward``."""
    if use_hip:       # (a multi-output spec: F and f_x [B,K] of ``hip_forward_multi`` for x [B,1])
        return lambda x: hip_forward(spec, None, x, h, nb_steps, multi=n_out_of(spec) > 1)[:2]
    f = (lambda x, hh: integrand.independant_forward(torch.cat((x, hh), 1))) if column else integrand
    return lambda x: (aten_forward(f, torch.zeros_like(x), x, h, nb_steps), f(x, h))


def host_solve(spec, h, target, nb_steps, lo, hi, tol, max_iter, scale=1., off=0., x_init=None):
    """Host-driven Newton loop over ``hip_forward`` (F and f_x in one launch per iteration): what runs when the library
    answers UMNN_EUNSUPPORTED for the in-kernel solve.  ``target`` [B,d], ``h`` [B,E*d] -> (x, f_x, status), each [B,d]."""
    with torch.no_grad():
        return newton_solve(quadrature_eval(spec, None, h, nb_steps, True), target, scale, off, lo, hi, tol, max_iter, x_init=x_init)


def aten_solve(integrand, h, target, nb_steps, lo, hi, tol, max_iter, scale=1., off=0., x_init=None):
    """Generic ATen path of the inverse (CPU tensors, float64, integrands ``mlp_spec`` does not recognise): the same
    algorithm on ``aten_forward``."""
    with torch.no_grad():
        out = newton_solve(quadrature_eval(None, integrand, h, nb_steps, False), target, scale, off, lo, hi, tol, max_iter, x_init=x_init)
    _state.path = "aten"
    return out


def solve_integral(spec, t, h, nb_steps, lo, hi, tol, max_iter):
    """x with int_0^x f(s; h) ds = t on the HIP path: one in-kernel solve per dimension, or the host-driven loop for nets the
    solve kernels do not cover.  ``t`` [B,d], ``h`` [B,E*d] -> (x, f_x, status), each [B,d] (x, f_x in t's dtype)."""
    B, d = t.shape
    t32, h32 = _f32c(t), _f32c(h)
    with torch.no_grad():
        x = torch.empty_like(t32)
        fx = torch.empty_like(t32)
        status = torch.empty(B, d, device=t.device, dtype=torch.int32)
        for j in range(d):
            out = hip_solve(spec, h32, t32, nb_steps, j=j, lo=lo, hi=hi, tol=tol, max_iter=max_iter, x_out=x) if B > 0 else (x, fx, status)
            if out is None:
                x, fx, status = host_solve(spec, h32, t32, nb_steps, lo, hi, tol, max_iter)
                break
            if B > 0:
                fx[:, j], status[:, j] = out[1], out[2]
    return x.to(t.dtype), fx.to(t.dtype), status


def newton_solve_sum(eval_fn, target, coef, lo, hi, tol, max_iter):
    """``newton_solve`` on a weighted sum of K monotone curves: sum_k coef[b,k] F_k(x_b) = target[b], where ``eval_fn(x [B,1]) ->
    (F [B,K], f [B,K])``.  -> (x [B,1], F [B,K], f [B,K], status [B,1]), F and f at the returned x (one more evaluation).  A
    non-finite F_k marks its row SOLVE_NONFINITE under a zero coefficient too (0 * inf is a NaN), like the kernel."""
    def sums(x):
        F, f = eval_fn(x)
        return (coef * F).sum(1, keepdim=True), (coef * f).sum(1, keepdim=True)

    with torch.no_grad():
        x, _, status = newton_solve(sums, target, 1., 0., lo, hi, tol, max_iter)
        F, f = eval_fn(x)
    return x, F, f, status


def solve_sum(spec, integrand, t, coef, h, nb_steps, lo, hi, tol, max_iter):
    """x [B,1] with sum_k coef[b,k] int_0^x f_k(s; h_b) ds = t[b] -> (x, F, f_x, status): F, f_x [B,K] at x in t's dtype, status
    [B,1] int32.  ``spec`` (the HIP path): the in-kernel solve of umnn_cc_solve_multi, or -- for nets whose images exceed the LDS,
    after a one-time notice -- ``newton_solve_sum`` over ``hip_forward_multi``, one launch per iteration.  ``spec`` None: the same
    iteration on the ATen quadrature of ``integrand`` (CPU tensors, float64, integrands ``mlp_spec`` does not recognise)."""
    if t.shape[0] == 0:
        return t.new_empty(t.shape), t.new_empty(coef.shape), t.new_empty(coef.shape), t.new_empty(t.shape, dtype=torch.int32)
    if spec is None:
        out = newton_solve_sum(quadrature_eval(None, integrand, h.detach(), nb_steps, False), t.detach(), coef.detach(), lo, hi, tol,
                               max_iter)
        _state.path = "aten"
        return out
    t32, c32, h32 = _f32c(t), _f32c(coef), _f32c(h)
    with torch.no_grad():
        out = hip_solve_multi(spec, h32, t32, c32, nb_steps, lo, hi, tol, max_iter)
        if out is None:
            out = newton_solve_sum(quadrature_eval(spec, None, h32, nb_steps, True), t32, c32, lo, hi, tol, max_iter)
    x, F, fx, status = out
    return x.to(t.dtype), F.to(t.dtype), fx.to(t.dtype), status


_row_counters = {}     # (device index, stream handle) -> zeroed uint32 [>= B] arrival counters (kernel leaves them zero)


def _counters(B, device, stream_handle):
    """Row-arrival counters of the one-pass log-likelihood.  Eager calls share one zeroed buffer per (device, stream): the
    finishing wave of every row resets its counter, so the buffer is all-zero again when the launch retires.  Under a
    hipGraph capture nothing may be created-and-cached (a tensor born in a capture lives in that graph's private pool and
    its zero-fill is a captured node, not an executed one): ``compute_ll`` asks ``fresh_counters`` for a buffer per captured
    call instead, whose memset is then part of every replay of that graph."""
    key = (device.index, stream_handle)
    t = _row_counters.get(key)
    if t is None or t.numel() < B:
        assert not torch.cuda.is_current_stream_capturing()
        t = _row_counters[key] = torch.zeros(max(B, 1024), dtype=torch.int32, device=device)
    return t


def ll_counters(B, device):
    """Counter buffer for one ``UMNNMAFFlow.compute_ll`` call on the current stream (see _counters)."""
    if torch.cuda.is_current_stream_capturing():
        return torch.zeros(B, dtype=torch.int32, device=device)        # this graph's own buffer and memset node
    return _counters(B, device, torch.cuda.current_stream(device).cuda_stream)


def hip_flow_ll_block(spec, x, h, scaling, nb_steps, reverse_z, first, last, ll, scratch, cnt=None):
    """One link of UMNNMAFFlow.compute_ll with the whole log-likelihood arithmetic inside the launch
    (umnn_flow_ll_block_forward): -> z; ``ll`` [B] is updated in place, ``scratch`` [B,d] is this launch's own; ``cnt`` the
    zeroed int32 [>= B] row-arrival counters (``ll_counters``; the launch leaves them zero)."""
    lib = _lib.lib()
    B, d, E = _shape(spec, x, h)
    z = torch.empty_like(x)
    w, s = device_tables(nb_steps, x.device)
    desc, keep = _desc(spec)
    with torch.cuda.device(x.device):
        if cnt is None:
            cnt = ll_counters(B, x.device)
        rc = lib.umnn_flow_ll_block_forward(ctypes.byref(desc), _ptr(x), _ptr(h), _ptr(scaling), _ptr(w), _ptr(s),
                                            int(nb_steps), B, d, E, 1 if reverse_z else 0, 1 if first else 0,
                                            1 if last else 0, _ptr(z), _ptr(scratch), _ptr(ll), _ptr(cnt),
                                            _stream(x.device))
    _lib.check(rc, "umnn_flow_ll_block_forward")
    _state.path = "hip"
    return z


# ----------------------------------------------------------------------------------------------
# generic ATen path (arbitrary callables; any device)
# ----------------------------------------------------------------------------------------------
_CHUNK_ELEMS = 1 << 24      # cap on rows*columns of the largest temporary per chunk of nodes


def _node_chunks(nb_steps, rows, cols):
    per = max(1, min(nb_steps + 1, _CHUNK_ELEMS // max(1, rows * cols)))
    return [(a, min(a + per, nb_steps + 1)) for a in range(0, nb_steps + 1, per)]


def _eval_chunk(integrand, x0, span, h, u):
    """Evaluate the integrand at nodes t = x0 + span*u_c/2 for a chunk of C nodes -> ([C,B,dout], h_rep)."""
    C, B = u.shape[0], x0.shape[0]
    t = (x0.unsqueeze(0) + span.unsqueeze(0) * u.view(C, 1, 1) / 2).reshape(C * B, -1)
    h_rep = h.unsqueeze(0).expand(C, -1, -1).reshape(C * B, -1)
    return t, h_rep


def aten_forward(integrand, x0, x, h, nb_steps, inv_f=False):
    """[B,d] for an integrand that returns one value per (row, dimension); [B,K] for a multi-output integrand (K values per row,
    x [B,1]): the CPU implementation of the multi-output feature."""
    w, s = device_tables(nb_steps, x.device)
    w, u = w.to(x.dtype), s.to(x.dtype) + 1
    span = x - x0
    total = None
    B, d = x.shape
    for a, b in _node_chunks(nb_steps, B, h.shape[1] + x.shape[1]):
        t, h_rep = _eval_chunk(integrand, x0, span, h, u[a:b])
        f = integrand(t, h_rep)
        if inv_f:
            f = 1 / f
        f = f.view(b - a, B, -1)
        if total is None:
            if f.shape[2] != d:
                _check_multi_x(f.shape[2], x)
            total = torch.zeros(B, f.shape[2], dtype=x.dtype, device=x.device)
        total = total + (f * w[a:b].view(-1, 1, 1)).sum(0)
    _state.path = "aten"
    return total * (span if total.shape[1] == d else span.expand(B, total.shape[1])) / 2


def _check_cumulate(values, x0, x, n):
    B = values.shape[0]
    if values.dim() != 3 or values.shape[1] != n + 1 or x.shape != (B, 1) or (x0 is not None and x0.shape != (B, 1)):
        raise RuntimeError(f"umnn_amd: cumulate takes values [B, nb_steps + 1, K] and limits [B, 1]; got {tuple(values.shape)} and "
                           f"{tuple(x.shape)} at nb_steps = {n}")


def _curve_abscissae(x0, x, nb_steps):
    """[B, nb_steps + 1]: the quadrature nodes of [x0, x] ASCENDING from x0 to x, in the kernels' rounding order
    x0 + ((x - x0) (s_j + 1)) / 2, the last one x itself (node 0 of the kernels)."""
    _, s = device_tables(nb_steps, x.device)
    u = (s.to(x.dtype) + 1).flip(0)
    t = x0 + (x - x0) * u.view(1, -1) / 2
    return torch.cat((t[:, :-1], x), 1)


def aten_cumulate(values, x0, x, nb_steps, ascending=True):
    """``hip_cumulate`` as one einsum with the cumulative matrix in values' dtype (float64 stays float64): any device, differentiable
    by plain autograd.  -> [B, nb_steps + 1, K], ascending."""
    _check_cumulate(values, x0, x, int(nb_steps))
    Q = device_cumulative_matrix(nb_steps, values.device, ascending, values.dtype).flip(0)
    span = x if x0 is None else x - x0
    return torch.einsum("ij,bjk->bik", Q, values) * (span.to(values.dtype) / 2).unsqueeze(2)


def aten_curve(integrand, x0, x, h, nb_steps):
    """The curve on ATen -> (t [B, n+1], C [B, n+1, K], f [B, n+1, K]), all ascending from x0 to x: the integrand at the nodes as
    ``aten_forward`` evaluates them (in node chunks), kept, and the cumulative matrix applied with one einsum.  Any device and dtype;
    differentiable through x0, x, h and every parameter by plain autograd."""
    B, n = x.shape[0], int(nb_steps)
    t = _curve_abscissae(x0, x, n)
    parts = []
    for a, b in _node_chunks(n, B, h.shape[1] + 1):
        hh = h.unsqueeze(1).expand(B, b - a, h.shape[1]).reshape(B * (b - a), -1)
        parts.append(integrand(t[:, a:b].reshape(B * (b - a), 1), hh).view(B, b - a, -1))
    f = torch.cat(parts, 1)
    C = aten_cumulate(f, x0, x, n)
    _state.path = "aten"
    return t, C, f


def aten_cumulate_adjoint(g, nb_steps, ascending=False):
    """``hip_cumulate_adjoint`` as one einsum with the adjoint table in g's dtype: any device."""
    return torch.einsum("ji,bik->bjk", device_cumulative_adjoint(nb_steps, g.device, ascending, g.dtype), g)


def _backward_switch(backward):
    if backward not in ("aten", "hip"):
        raise ValueError(f"umnn_amd: backward must be 'aten' or 'hip'; got {backward!r}")
    return backward == "hip"


def cumulate(values, x0, x, nb_steps, backward="aten"):
    """Cumulative quadrature of values given at the ascending nodes of [x0, x] (``curve``'s t): [B, n+1, K] -> the integral from x0
    to every node, [B, n+1, K], index 0 exactly 0.  One ``umnn_cc_cumulate`` launch for GPU tensors of K <= 16 outputs when nothing
    asks for a gradient (recorded: ``umnn::cc_cumulate``); ``aten_cumulate`` otherwise -- host tensors, float64, K > 16, nb_steps
    beyond the kernel's table budget, and, with ``backward="aten"`` (the default), whenever an input requires grad.
    ``backward="hip"``: the same launch under autograd too (``CumulateFunction``: its backward is one ``umnn_cc_cumulate_adjoint``
    launch, a, and d values = (x - x0)/2 a, dx = 1/2 sum a values, dx0 = -dx); what the kernel does not take runs ``aten_cumulate``
    as before, never an error."""
    hip_grad = _backward_switch(backward)
    wants_graph = torch.is_grad_enabled() and any(t is not None and t.requires_grad for t in (values, x0, x))
    hip = (values.is_cuda and values.dtype in (torch.float32, torch.bfloat16, torch.float16) and values.dim() == 3
           and 1 <= values.shape[2] <= _lib.MAX_OUTPUTS and not (wants_graph and not hip_grad))
    if hip and wants_graph:
        if _graph_mode() or (not getattr(_state, "force_generic", False) and _cumulate_kernel_ok(values.shape[2], nb_steps, adjoint=True)):
            return CumulateFunction.apply(values, x0, x, int(nb_steps))
        hip = False
    if hip and _graph_mode():
        return torch.ops.umnn.cc_cumulate(values, x0, x, int(nb_steps), True)
    if hip and not getattr(_state, "force_generic", False) and _cumulate_kernel_ok(values.shape[2], nb_steps):
        return hip_cumulate(values, x0, x, nb_steps, ascending=True)
    out = aten_cumulate(values, x0, x, nb_steps)
    _state.path = "aten"
    return out


def _cumulate_kernel_ok(K, nb_steps, adjoint=False):
    """One zero-row call (it launches nothing) of the entry the caller is about to use: ``adjoint`` on the route that differentiates."""
    lib = _lib.lib()
    if adjoint:
        name, rc = "umnn_cc_cumulate_adjoint", lib.umnn_cc_cumulate_adjoint(None, None, int(nb_steps), 0, int(K), None, None)
    else:
        name, rc = "umnn_cc_cumulate", lib.umnn_cc_cumulate(None, None, None, None, int(nb_steps), 0, int(K), None, None)
    if rc == _lib.EUNSUPPORTED:
        _warn_once(("cumulate-aten", int(nb_steps)), f"umnn_amd: no HIP cumulate kernel at nb_steps = {int(nb_steps)} "
                   f"({_lib.lib().umnn_last_error().decode('utf-8', 'replace')}): one einsum on the GPU instead.")
        return False
    _lib.check(rc, name)
    return True


class CumulateFunction(torch.autograd.Function):
    """``cumulate(..., backward="hip")`` under autograd: the forward launch, and a backward that is the adjoint launch plus the span
    factor.  Values ascending, as ``cumulate`` takes them."""

    @staticmethod
    def forward(ctx, values, x0, x, nb_steps):
        ctx.nb_steps, ctx.x0_none, ctx.graph = int(nb_steps), x0 is None, _graph_mode()
        if ctx.graph:
            out = torch.ops.umnn.cc_cumulate(values, x0, x, ctx.nb_steps, True)
        else:
            out = hip_cumulate(values, x0, x, ctx.nb_steps, ascending=True)
        ctx.save_for_backward(values, x, *(() if x0 is None else (x0,)))
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        values, x, *lims = ctx.saved_tensors
        nig = ctx.needs_input_grad
        g32 = g.float().contiguous()
        a = torch.ops.umnn.cc_cumulate_adjoint(g32, ctx.nb_steps, True) if ctx.graph else hip_cumulate_adjoint(g32, ctx.nb_steps, True)
        span = x.float() if ctx.x0_none else x.float() - lims[0].float()
        dv = (a * (span / 2).unsqueeze(2)).to(values.dtype) if nig[0] else None
        dx = dx0 = None
        if nig[1] or nig[2]:
            dx = (a * values.float()).sum((1, 2)).unsqueeze(1) / 2
            dx0 = (-dx).to(lims[0].dtype) if (nig[1] and not ctx.x0_none) else None
            dx = dx.to(x.dtype) if nig[2] else None
        return dv, dx0, dx, None


def _curve_launches(spec, x0, x, h, nb_steps):
    """The two launches of a curve on fp32 copies of the inputs -> (t, C, f_nodes, x0 or None, x, h): t and C ascending, f_nodes in
    node order; recorded as the two ops.  (bf16 / fp16 callers: fp32 from end to end -- the node values are rounded once, outside.)"""
    x0z = torch.zeros_like(x) if x0 is None else x0
    x0, x0z, x, h = (None if x0 is None else x0.float()), x0z.float(), x.float(), h.float()
    if _graph_mode():
        _, f_nodes = torch.ops.umnn.cc_forward_multi_nodes(x0, x, h, *spec_args(spec), int(nb_steps))
        C = torch.ops.umnn.cc_cumulate(f_nodes, x0, x, int(nb_steps), False)
    else:
        _, f_nodes = hip_forward_multi_nodes(spec, x0, x, h, nb_steps)
        C = hip_cumulate(f_nodes, x0, x, nb_steps)
    return _curve_abscissae(x0z, x, nb_steps), C, f_nodes, x0, x, h


def curve(spec, integrand, x0, x, h, nb_steps):
    """The whole monotone curve from ONE quadrature's worth of integrand evaluations -> (t [B, n+1], C [B, n+1, K], f [B, n+1, K]),
    all ascending: t the n + 1 Clenshaw-Curtis nodes of [x0, x] (t[:, 0] = x0, t[:, n] = x), C[:, i, k] = int_{x0}^{t_i} f_k(s; h) ds
    (C[:, 0] = 0 exactly, C[:, n] the integral ``aten_forward`` / the forward kernels return, up to rounding) and f the integrand there.
    ``spec`` (``_hip_spec``: an MLP of 1..16 outputs on GPU tensors): two launches, the forward that keeps its node values and
    ``umnn_cc_cumulate`` (recorded: ``umnn::cc_forward_multi_nodes`` and ``umnn::cc_cumulate``) -- unless the library answers
    UMNN_EUNSUPPORTED (announced once), which runs ``aten_curve`` like ``spec`` None does: CPU tensors, float64, n_out > 16,
    integrands ``mlp_spec`` does not recognise.  The kernels record no autograd graph: callers that need gradients pass ``spec``
    None, or go through ``CurveFunction`` (``IntegralCurve`` decides)."""
    if spec is None or not (_graph_mode() or _curve_kernels_ok(spec, nb_steps)):
        return aten_curve(integrand, torch.zeros_like(x) if x0 is None else x0, x, h, nb_steps)
    with torch.no_grad():
        out_dtype = x.dtype
        t, C, f_nodes = _curve_launches(spec, x0, x, h, nb_steps)[:3]
        return tuple(v.to(out_dtype) for v in (t, C, f_nodes.flip(1)))


def aten_vjp_nodes(integrand, x0, x, h, cot_nodes, nb_steps):
    """``hip_backward_multi_nodes`` on ATen -> (dx0_tau, dx_tau, dh, dtheta): the VJP of f at the nodes t_j = x0 + (x - x0) u_j / 2
    (node 0 is x itself) for the cotangent cot_nodes [B, n+1, K] in node order, in node chunks, through ``torch.func.vjp`` over the
    pure form of the integrand like ``aten_vjp``; the cotangent tau_j of t_j that the same VJP returns is handed to the limits,
    dx_tau = sum_j (u_j / 2) tau_j and dx0_tau = sum_j (1 - u_j / 2) tau_j.  dtheta is flat, in parameters() order, None for an
    integrand without parameters.  Any device and dtype."""
    f, params = _pure(integrand)
    _, s = device_tables(nb_steps, x.device)
    u = s.to(x.dtype) + 1
    with torch.no_grad():
        B = x.shape[0]
        _check_multi_x(cot_nodes.shape[2], x)
        span = x - x0
        d_params = [torch.zeros_like(p) for p in params]
        dh, dx, dx0 = torch.zeros_like(h), torch.zeros_like(x), torch.zeros_like(x)
        for a, e in _node_chunks(nb_steps, B, h.shape[1] + 1):
            t, h_rep = _eval_chunk(None, x0, span, h, u[a:e])
            if a == 0:
                t = torch.cat((x, t[B:]), 0)                 # node 0 is x itself, as in the kernels
            val, vjp = torch.func.vjp(f, params, t, h_rep)
            gp, gt, gh = vjp(cot_nodes[:, a:e].transpose(0, 1).reshape(val.shape))
            for acc, gr in zip(d_params, gp):
                acc += gr
            dh += gh.view(e - a, B, -1).sum(0)
            tau, hu = gt.view(e - a, B, 1), (u[a:e] / 2).view(-1, 1, 1)
            dx += (tau * hu).sum(0)
            dx0 += (tau * (1 - hu)).sum(0)
    _state.path = _last_backward["path"] = "aten"
    return dx0, dx, dh, (_flatten(d_params) if d_params else None)


def curve_vjp(x0, x, f_nodes, gt, gC, gf, nb_steps, need, adjoint, vjp_nodes):
    """The backward of a curve from its pieces -> (dx0, dx, dh, dtheta_flat), None where ``need`` says so.  gt [B, n+1], gC and gf
    [B, n+1, K] are the cotangents of (t, C, f), ascending like them; f_nodes the saved node values in NODE order; x0 None: zeros.
    ``adjoint(gC)`` -> a in node order (the adjoint cumulate without its span factor), ``vjp_nodes(cot)`` -> (dx0_tau, dx_tau, dh,
    dtheta) (``hip_backward_multi_nodes`` / ``aten_vjp_nodes``).  With span = x - x0 and u ascending from 0 to 2:

        cot = span/2 a + gf          S = 1/2 sum_jk a f          dx  = dx_tau  + sum_j gt_j u_j/2       + S
                                                                 dx0 = dx0_tau + sum_j gt_j (1 - u_j/2) - S

    the exact gradient of the DISCRETISED curve (every node moves with both limits), which is what autograd gives through
    ``aten_curve`` -- not the Leibniz convention dF/dx = f(x) of the scalar quadrature operators.  No division by span: a row with
    x == x0 is an ordinary row."""
    span = x if x0 is None else x - x0
    a = adjoint(gC.contiguous())
    cot = torch.addcmul(gf.flip(1), a, (span / 2).unsqueeze(2))
    dx0, dx, dh, dtheta = vjp_nodes(cot)
    if need[0] or need[1]:
        _, s = device_tables(nb_steps, x.device)
        hu = ((s.to(x.dtype) + 1) / 2).flip(0).view(1, -1)
        S = (a * f_nodes).sum((1, 2)).unsqueeze(1) / 2
        dx = dx + (gt * hu).sum(1, keepdim=True) + S if need[1] else None
        dx0 = dx0 + (gt * (1 - hu)).sum(1, keepdim=True) - S if need[0] else None
    return (dx0 if need[0] else None, dx if need[1] else None, dh if need[2] else None, dtheta if need[3] else None)


class CurveFunction(torch.autograd.Function):
    """The curve on the HIP kernels under autograd (``IntegralCurve.apply(..., backward="hip")``): forward the two evaluation launches,
    bit for bit; backward one ``umnn_cc_cumulate_adjoint`` launch, the elementwise glue of ``curve_vjp`` in torch ops and the
    passes of ``umnn_cc_backward_multi_nodes``.  Recorded: ``umnn::cc_cumulate_adjoint`` and ``umnn::cc_backward_multi_nodes``,
    which make the HIP / ATen choice when they run.  ``flat_params`` receives d_theta, as in ``ParallelNeuralIntegral``."""

    @staticmethod
    def forward(ctx, x0, x, integrand, flat_params, h, nb_steps):
        spec = _hip_spec(integrand, x, multi=True, who="IntegralCurve")
        ctx.nb_steps, ctx.x0_none = int(nb_steps), x0 is None
        ctx.dtypes = (None if x0 is None else x0.dtype, x.dtype, h.dtype)
        t, C, f_nodes, x0f, xf, hf = _curve_launches(spec, x0, x, h, nb_steps)
        lims = () if x0 is None else (x0f,)
        if not _graph_mode():       # clones: callers may write their limits in place after the call (as ``_quad_forward`` assumes)
            lims, xf = tuple(v.clone() if v is x0 else v for v in lims), (xf.clone() if xf is x else xf)
        _save(ctx, spec, integrand, *lims, xf, hf, f_nodes)
        return tuple(v.to(x.dtype) for v in (t, C, f_nodes.flip(1)))

    @staticmethod
    @once_differentiable
    def backward(ctx, gt, gC, gf):
        nig = ctx.needs_input_grad
        n = 3 if ctx.x0_none else 4
        tensors, net = _saved(ctx, n)
        x0, (x, h, f_nodes) = (None if ctx.x0_none else tensors[0]), tensors[n - 3:n]
        need = [bool(nig[0]) and x0 is not None, bool(nig[1]), bool(nig[4]), bool(nig[3])]
        steps = ctx.nb_steps
        if net:
            def adjoint(g):
                return torch.ops.umnn.cc_cumulate_adjoint(g, steps, False)

            def vjp_nodes(cot):
                return torch.ops.umnn.cc_backward_multi_nodes(x0, x, h, cot, *net, steps, need)
        else:
            spec = ctx.spec

            def adjoint(g):
                return hip_cumulate_adjoint(g, steps)

            def vjp_nodes(cot):
                return hip_backward_multi_nodes(spec, x0, x, h, cot, steps, need)
        dx0, dx, dh, dtheta = curve_vjp(x0, x, f_nodes, gt.float(), gC.float(), gf.float(), steps, need, adjoint, vjp_nodes)
        d0, d1, d2 = ctx.dtypes
        return (None if dx0 is None else dx0.to(d0), None if dx is None else dx.to(d1), None, dtheta,
                None if dh is None else dh.to(d2), None)


def _note_aten_backward(grad):
    _last_backward["path"] = "aten"


class IntegralCurve:
    """(t, C, f) = the curve of int_{x0}^{t} f(s; h) ds at the n + 1 quadrature nodes of [x0, x] (``curve``):

        IntegralCurve.apply(x0, x, integrand, flat_params, h, nb_steps=20, backward="aten") -> (t [B, n+1], C [B, n+1, K], f [B, n+1, K])

    x [B,1]; x0 [B,1] or None (zeros); the calling convention of the quadrature operators.  The HIP kernels evaluate the curve when
    grad mode is off or nothing -- x0, x, h, a parameter of the integrand -- requires grad.  When something does:

      * ``backward="aten"`` (the default): ``aten_curve`` under plain autograd on the tensors' device, announced once; ``flat_params``
        is accepted for parity and not read.
      * ``backward="hip"``: ``CurveFunction`` -- the same two launches forward (t, C, f bit for bit those of the ``no_grad`` call), and
        a once-differentiable backward on the kernels, one adjoint-cumulate launch and the passes of the multi-output backward with a
        cotangent per node.  ``flat_params`` (``_flatten(integrand.parameters())``) receives d_theta, as in ``ParallelNeuralIntegral``:
        an integrand with trainable parameters and no ``flat_params`` that requires grad stays on ATen.  CPU tensors, float64,
        n_out > 16, nb_steps > 127 and nets beyond the LDS run ``aten_curve`` under autograd exactly as with ``"aten"``, with the
        usual one-time notice, never an error.

    ``backward_path_taken()`` reports the route of the most recent curve backward, "hip" or "aten" (on the ATen route through a
    hook on the outputs that leaves their gradients alone).  Both give the exact gradient of the DISCRETISED curve (``curve_vjp``): every node moves with both limits.  That is deliberately
    not the Leibniz convention dF/dx = f(x) of the scalar quadrature operators."""

    @staticmethod
    def apply(x0, x, integrand, flat_params, h, nb_steps=20, backward="aten"):
        hip_grad = _backward_switch(backward)
        if x.dim() != 2 or x.shape[1] != 1:
            raise RuntimeError(f"umnn_amd: a curve is integrated over x of shape [B, 1]; got {tuple(x.shape)}")
        trainable = isinstance(integrand, torch.nn.Module) and any(p.requires_grad for p in integrand.parameters())
        wants_graph = torch.is_grad_enabled() and (any(t is not None and t.requires_grad for t in (x0, x, h)) or trainable)
        spec = _hip_spec(integrand, x, multi=True, who="IntegralCurve")
        if spec is not None and wants_graph:
            if hip_grad and trainable and (flat_params is None or not flat_params.requires_grad):
                _warn_once("curve-grad-flat", "umnn_amd: IntegralCurve(backward='hip') hands the parameters' gradient to flat_params; "
                                              "without one that requires grad the curve runs on the generic ATen path under autograd.")
            elif hip_grad and (_graph_mode() or _curve_grad_kernels_ok(spec, nb_steps)):
                return CurveFunction.apply(x0, x, integrand, flat_params, h, int(nb_steps))
            elif not hip_grad and not _graph_mode():
                _warn_once("curve-grad", "umnn_amd: a curve whose inputs require grad runs on the generic ATen path under autograd "
                                         "(the HIP curve kernels are the evaluation path; use torch.no_grad() for them).")
            spec = None
        with torch.set_grad_enabled(wants_graph):
            out = curve(spec, integrand, x0, x, h, nb_steps)
        # plain autograd runs this backward: a hook on each output (a loss may use any one of them) lets ``backward_path_taken()``
        # report it; the hooks return nothing, so the gradients are autograd's own
        if wants_graph and not _graph_mode():
            for v in out:
                if v.requires_grad:
                    v.register_hook(_note_aten_backward)
        return out


def _pure(integrand):
    """``integrand`` as a pure function of its parameters -> (f(params, t, h), params): a module through ``functional_call`` on its
    detached ``parameters()``; any other callable with an empty parameter list; a pair that already is one (the ops' W[] / b[]
    adapter, ``ops.pure_mlp``) as it is."""
    if isinstance(integrand, tuple):
        return integrand
    if hasattr(integrand, "_umnn_pure"):          # (a module that is a VIEW of another's parameters: monotonic.OutputRow)
        return integrand._umnn_pure()
    if isinstance(integrand, torch.nn.Module):
        names = [n for n, _ in integrand.named_parameters()]
        return (lambda ps, t, h: torch.func.functional_call(integrand, dict(zip(names, ps)), (t, h)),
                [p.detach() for p in integrand.parameters()])
    return (lambda ps, t, h: integrand(t, h)), []


def aten_vjp(integrand, x0, x, h, g, g_fx, nb_steps, inv_f=False, limits=True):
    """THE ATen quadrature backward -> (dx0, dx, dh, dtheta): the VJP of f over all nodes with cotangent g (x - x0)/2 w_k for the
    parameters and h, in node chunks; with ``g_fx`` the VJP of f(x; h) for the cotangent of the f_x output on top; the Leibniz terms
    dx = f(x) g and dx0 = -f(x0) g (None unless ``limits``).  dtheta is flat, in parameters() order, None for an integrand without
    parameters.  ``torch.func.vjp`` over the pure form of the integrand (``_pure``), so the same code runs inside a
    ``once_differentiable`` backward and inside an op kernel below autograd, where ``torch.autograd.grad`` records nothing."""
    f, params = _pure(integrand)
    w, s = device_tables(nb_steps, x.device)
    w, u = w.to(x.dtype), s.to(x.dtype) + 1
    with torch.no_grad():
        span = x - x0
        B, d = x.shape
        multi = g.shape[1] != d          # g [B,K] of a multi-output integrand over x [B,1]: dx / dx0 are sums over k
        if multi:
            _check_multi_x(g.shape[1], x)
        cot = g * (span.expand(B, g.shape[1]) if multi else span) / 2
        d_params = [torch.zeros_like(p) for p in params]
        dh = torch.zeros_like(h)
        for a, e in _node_chunks(nb_steps, B, h.shape[1] + x.shape[1]):
            t, h_rep = _eval_chunk(None, x0, span, h, u[a:e])

            def f_nodes(ps, hr, t=t):
                v = f(ps, t, hr)
                return 1 / v if inv_f else v

            val, vjp = torch.func.vjp(f_nodes, params, h_rep)
            gp, gh = vjp((cot.unsqueeze(0) * w[a:e].view(-1, 1, 1)).reshape(val.shape))
            for acc, gr in zip(d_params, gp):
                acc += gr
            dh += gh.view(e - a, B, -1).sum(0)
        dx0 = dx = None
        over_k = (lambda t: t.sum(1, keepdim=True)) if multi else (lambda t: t)      # the Leibniz terms of K outputs add up
        if g_fx is not None:
            fx, vjp = torch.func.vjp(f, params, x, h)
            gp, gx, gh = vjp(g_fx)
            dx, dh = over_k(fx * g) + gx, dh + gh
            d_params = [acc + gr for acc, gr in zip(d_params, gp)]
        elif limits:
            dx = over_k(f(params, x, h) * g)
        if limits:
            dx0 = over_k(-f(params, x0, h) * g)
    _state.path = _last_backward["path"] = "aten"
    return dx0, dx, dh, (_flatten(d_params) if d_params else None)


def aten_backward(integrand, x0, x, h, g, nb_steps, inv_f=False):
    """(d_theta, d_h) of ``aten_vjp``: what ``integrate(compute_grad=True)`` returns."""
    _, _, dh, dtheta = aten_vjp(integrand, x0, x, h, g, None, nb_steps, inv_f, limits=False)
    return dtheta, dh


def quadrature_backward(spec, integrand, x0, x, h, g, g_fx, nb_steps, need=(True, True, True, True), inv_f=False, z2_saved=None,
                        h0_cot=None):
    """The quadrature backward of every operator -> (dx0, dx, dh, dtheta_flat), None where ``need`` says so: the HIP kernels when
    ``spec`` (None: the forward ran on ATen) has a backward kernel, else ``aten_vjp`` on ``integrand``.  x0 None: lower limit 0.
    ``h0_cot`` [B,d] (single-output operators): a flow block's h_0 term, added to embedding row 0 of dh -- inside the HIP launch that
    stores dh, in fp32 torch ops on the ATen path."""
    need = (bool(need[0]) and x0 is not None, bool(need[1]), bool(need[2]), bool(need[3]))
    multi = spec is not None and n_out_of(spec) > 1
    if spec is not None and (_multi_kernels_ok(spec) if multi else _hip_backward_ok(spec, x, h)):
        return hip_backward(spec, x0, x, h, g, g_fx, nb_steps, need, inv_f, z2_saved, h0_cot, multi)
    out = aten_vjp(integrand, torch.zeros_like(x) if x0 is None else x0, x, h, g, g_fx, nb_steps, inv_f, limits=need[0] or need[1])
    out = tuple(t if n else None for t, n in zip(out, need))
    if h0_cot is not None and out[2] is not None:
        out = (out[0], out[1], _add_h0(out[2], h0_cot, x.shape[1]), out[3])
    return out


def split_flat(flat, shapes, needed):
    """Flat d_theta -> views of ``shapes`` in parameters() order (W_0, b_0, W_1, ...), None where not ``needed``: no narrow + copy
    per parameter."""
    grads, o = [], 0
    for shp, n in zip(shapes, needed):
        k = int(torch.Size(shp).numel())
        grads.append(flat[o:o + k].view(shp) if (n and flat is not None) else None)
        o += k
    return grads


# ----------------------------------------------------------------------------------------------
# the seam: a ctypes launch, or -- while a graph is recorded -- the torch.ops.umnn op of the same launch
# ----------------------------------------------------------------------------------------------
def spec_args(spec):
    """MlpSpec -> (W[], b[], hidden_act, out_act): the integrand as the ops take it."""
    return [l.weight for l in spec.linears], [l.bias for l in spec.linears], spec.hidden_act, spec.out_act


def cc_forward(spec, x0, x, h, nb_steps, inv_f=False):
    """-> (F, f_x).  Recorded: ``umnn::cc_forward``, differentiable through the op.  A multi-output spec: (F, f_x) [B, n_out] of
    ``hip_forward_multi`` / ``umnn::cc_forward_multi``."""
    multi = n_out_of(spec) > 1
    if _graph_mode():
        op = torch.ops.umnn.cc_forward_multi if multi else torch.ops.umnn.cc_forward
        return op(x0, x, h, *spec_args(spec), int(nb_steps), bool(inv_f))
    return hip_forward(spec, x0, x, h, nb_steps, inv_f, multi)[:2]


def cc_forward_jac(spec, integrand, x0, x, h, nb_steps, no_graph):
    """(F, f_x) of a flow block whose epilogue is composed from torch ops: ``IntegralWithJacobianParams`` when a gradient can be
    asked for, the bare launch otherwise (``no_graph``)."""
    if no_graph or _graph_mode():
        return cc_forward(spec, x0, x, h, nb_steps)
    return IntegralWithJacobianParams.apply(x0, x, integrand, h, nb_steps, *integrand.parameters())


def flow_block(spec, integrand, x, h, scaling, nb_steps, reverse_z, log_jac_in, train):
    """(z, log_jac) of a block with the epilogue inside the launch.  ``train``: as ONE autograd node -- eager ``FlowBlockTransform``
    with its z_2 hand-off, recorded ``umnn::flow_block`` (whose backward recomputes z_2: never a different result)."""
    if _graph_mode():
        if train:
            x, h = x.contiguous(), h.contiguous()
        else:
            scaling = scaling.detach()          # (like the eager launch: no gradient for scaling on this path)
        return torch.ops.umnn.flow_block(x, h, scaling, *spec_args(spec), nb_steps, reverse_z, log_jac_in)[:2]
    if train:
        return FlowBlockTransform.apply(x.contiguous(), integrand, h.contiguous(), scaling, nb_steps, reverse_z, log_jac_in,
                                        *integrand.parameters())
    return hip_flow_block(spec, x, h, scaling, nb_steps, reverse_z, log_jac_in)[:2]


def flow_ll(z, log_jac):
    """Differentiable ll [B] from z and the summed log_jac: one launch per direction."""
    if _graph_mode():
        return torch.ops.umnn.flow_ll(z.contiguous(), log_jac.contiguous())
    return FlowLogLikelihood.apply(z, log_jac)


def flow_ll_workspace(x):
    """What the links of one one-pass log-likelihood share in eager mode -> (ll [B], scratch [B,d], row counters: under a hipGraph
    capture this call's own zeroed buffer); None while a graph is recorded, where every ``umnn::flow_ll_block`` owns its own."""
    if _graph_mode():
        return None
    return (torch.empty(x.shape[0], device=x.device, dtype=torch.float32), torch.empty_like(x), ll_counters(x.shape[0], x.device))


def flow_ll_link(spec, x, h, scaling, nb_steps, reverse_z, first, last, ll, work):
    """One link of the one-pass log-likelihood -> (z, running ll); ``ll`` None for the first link, ``work`` from ``flow_ll_workspace``."""
    if work is None:
        return torch.ops.umnn.flow_ll_block(x, h, scaling, *spec_args(spec), nb_steps, reverse_z, first, last, ll)
    ll, scratch, cnt = work
    return hip_flow_ll_block(spec, x, h, scaling, nb_steps, reverse_z, first, last, ll, scratch, cnt), ll


def hip_flow_block_cotangents(gz, glj, fx, scaling, reverse_z):
    """Cotangents of F and f_x of a flow block from those of z and log_jac (umnn_flow_block_cotangents) -> (gF, gfx or None)."""
    B, d = fx.shape
    gF, gfx = torch.empty_like(fx), (torch.empty_like(fx) if glj is not None else None)
    with torch.cuda.device(fx.device):
        rc = _lib.lib().umnn_flow_block_cotangents(_ptr(gz), _ptr(glj), _ptr(fx), _ptr(scaling), B, d, 1 if reverse_z else 0,
                                                   _ptr(gF), _ptr(gfx), _stream(fx.device))
    _lib.check(rc, "umnn_flow_block_cotangents")
    return gF, gfx


def flow_adjoint_update(g, r, log_jac, lam, tol, flags, out=None):
    """One adjoint Jacobi step: out = lam + (g - r) exp(-log_jac), all [B,d]; ``out`` may be ``lam`` itself (allocated when None).
    ``flags`` (int32 [1], zeroed by the caller) gets bit 0 when some |g - r| > tol max(1, |g|) and bit 1 when some g - r is not finite
    (such an entry never sets bit 0).  One launch of umnn_flow_adjoint_update for contiguous fp32 GPU tensors; the same arithmetic in
    torch ops for host tensors and other dtypes.  -> out"""
    if out is None:
        out = torch.empty_like(lam)
    if lam.is_cuda and all(t.dtype == torch.float32 and t.is_contiguous() for t in (g, r, log_jac, lam, out)) \
            and not getattr(_state, "force_generic", False):
        B, d = lam.shape
        with torch.cuda.device(lam.device):
            rc = _lib.lib().umnn_flow_adjoint_update(_ptr(g), _ptr(r), _ptr(log_jac), _ptr(lam), B, d, float(tol), _ptr(out), _ptr(flags),
                                                     _stream(lam.device))
        _lib.check(rc, "umnn_flow_adjoint_update")
        return out
    res = g - r
    bad = ~torch.isfinite(res)
    over = (res.abs() > tol * g.abs().clamp(min=1.)) & ~bad
    flags |= over.any().to(flags.dtype) + 2 * bad.any().to(flags.dtype)
    torch.add(lam, res * torch.exp(-log_jac), out=out)
    return out


def hip_flow_ll(z, log_jac):
    """ll [B] fp32 of a flow from its z and summed log_jac (umnn_flow_ll_forward)."""
    z, log_jac = z.contiguous(), log_jac.contiguous()
    B, d = z.shape
    ll = torch.empty(B, device=z.device, dtype=torch.float32)
    with torch.cuda.device(z.device):
        rc = _lib.lib().umnn_flow_ll_forward(_ptr(z), _ptr(log_jac), B, d, _ptr(ll), _stream(z.device))
    _lib.check(rc, "umnn_flow_ll_forward")
    return ll


def _glue_ok(*tensors):
    """One launch of a cc_flow_glue kernel serves these tensors: contiguous fp32 on the GPU, outside a recorded graph."""
    if _graph_mode():       # (first: traced code cannot read the thread-local switch below)
        return False
    return (tensors[0].is_cuda and all(t.dtype == torch.float32 and t.is_contiguous() for t in tensors)
            and not getattr(_state, "force_generic", False))


def sample_lj_rows(fx, scaling, lj_row=None):
    """Row sums of a block's log-Jacobian from the f(x) of its solves: ``lj_row`` [B] += sum_i (log(fx[b,i] + 1e-10) + scaling[i]), or
    a new tensor when ``lj_row`` is None.  One umnn_flow_sample_lj_rows launch for contiguous fp32 GPU tensors (fixed summation
    order); the same arithmetic in torch ops, in the tensors' dtype, otherwise.  -> lj_row"""
    B, d = fx.shape
    if _glue_ok(fx, scaling) and (lj_row is None or _glue_ok(lj_row)):
        first = lj_row is None
        if first:
            lj_row = torch.empty(B, device=fx.device, dtype=torch.float32)
        with torch.cuda.device(fx.device):
            rc = _lib.lib().umnn_flow_sample_lj_rows(_ptr(fx), _ptr(scaling), B, d, 1 if first else 0, _ptr(lj_row), _stream(fx.device))
        _lib.check(rc, "umnn_flow_sample_lj_rows")
        return lj_row
    s = (torch.log(fx + 1e-10) + scaling.to(fx.dtype).unsqueeze(0)).sum(1)
    return s if lj_row is None else lj_row + s


def sample_ll(z, lj_row, pi=None):
    """Log-density of drawn samples from the noise ``z`` [B,d] they were drawn from and the flow's summed log-Jacobian ``lj_row`` [B]:
    lj_row - 1/2 sum_i (log 2 pi + z_i^2).  One umnn_flow_sample_ll launch for contiguous fp32 GPU tensors, torch ops otherwise --
    with the flow's own ``pi`` buffer when given, the constant ``compute_ll`` uses (a float64 flow keeps the fp32-rounded value)."""
    if _glue_ok(z, lj_row):
        B, d = z.shape
        ll = torch.empty(B, device=z.device, dtype=torch.float32)
        with torch.cuda.device(z.device):
            rc = _lib.lib().umnn_flow_sample_ll(_ptr(z), _ptr(lj_row), B, d, _ptr(ll), _stream(z.device))
        _lib.check(rc, "umnn_flow_sample_ll")
        return ll
    log_2pi = math.log(2 * math.pi) if pi is None else torch.log(pi.to(z.dtype) * 2)
    return lj_row - .5 * (log_2pi + z ** 2).sum(1)


def hip_flow_ll_backward(z, g_ll, need_z, need_lj):
    """-> (gz, glj) of hip_flow_ll for the cotangent g_ll (umnn_flow_ll_backward); None where not needed."""
    B, d = z.shape
    g_ll = g_ll.contiguous()
    gz = torch.empty_like(z) if need_z else None
    glj = torch.empty_like(z) if need_lj else None
    with torch.cuda.device(z.device):
        rc = _lib.lib().umnn_flow_ll_backward(_ptr(z), _ptr(g_ll), B, d, _ptr(gz), _ptr(glj), _stream(z.device))
    _lib.check(rc, "umnn_flow_ll_backward")
    return gz, glj


def flow_block_vjp(spec, integrand, x, h, fx, scaling, gz, glj, nb_steps, reverse_z, need, z2_saved=None):
    """Backward of a fused block -> (dx, dh, dtheta_flat) for ``need``: one elementwise launch (cotangents of F and f_x from those of z
    and log_jac), and the quadrature backward, whose d_h kernel also adds the h_0 term (z carries h_0 = embedding row 0,
    UMNNMAF.py:80: the cotangent of F is that of h_0 too) before it stores d_h -- a bf16 d_h is rounded once, row 0 included."""
    gF, gfx = hip_flow_block_cotangents(gz, glj, fx, scaling, reverse_z)
    _, dx, dh, dtheta = quadrature_backward(spec, integrand, None, x, h, gF, gfx, nb_steps, (False, *need), z2_saved=z2_saved, h0_cot=gF)
    return dx, dh, dtheta


class FlowBlockTransform(torch.autograd.Function):
    """(z, log_jac) of one UMNN-MAF block on the TRAINING path as ONE autograd node (UMNNMAF.py:76-139):

        z[b, rev(i)] = exp(s_i) (int_0^{x_bi} f(t; h_b) dt + h_0[b,i]),     log_jac = [log_jac_in +] log(f(x; h) + 1e-10) + s

    forward = the fused-epilogue launch of the inference path (umnn_flow_stack_block_forward); backward = ``flow_block_vjp``.
    Composed from torch ops (exp, mul, add, log, add, flip, select and their backward nodes) the same
    arithmetic is ~15 launches and 8 autograd nodes per block.  Internal to the flow blocks: fp32 storage, lower limit 0, frozen
    ``scaling`` (UMNNMAF.py:53) -- anything else keeps the composed path."""

    @staticmethod
    def forward(ctx, x, integrand, h, scaling, nb_steps, reverse_z, log_jac_in, *params):
        spec = mlp_spec(integrand)
        ctx.spec, ctx.nb_steps, ctx.integrand, ctx.reverse_z = spec, nb_steps, integrand, bool(reverse_z)
        ctx.shapes = [p.shape for p in params]
        # (nets of the three-stage backward family: the forward leaves z_2 of every node for the backward, which then skips stage A)
        want_z2 = any(ctx.needs_input_grad[7:]) or ctx.needs_input_grad[0] or ctx.needs_input_grad[2]
        out = hip_flow_block(spec, x, h, scaling, nb_steps, reverse_z, log_jac_in, save_z2=want_z2)
        z, lj, fx = out[0], out[1], out[2]
        ctx.z2 = out[4] if want_z2 else None          # (save_z2=False returns four values: only log_jac_in needs a gradient)
        ctx.save_for_backward(x.clone(), h, fx, scaling)      # (x cloned: callers clamp z / reuse x in place, UMNNMAF.py:150)
        return z, lj

    @staticmethod
    @once_differentiable
    def backward(ctx, gz, glj):
        x, h, fx, scaling = ctx.saved_tensors
        nig = ctx.needs_input_grad
        gz = None if gz is None else gz.contiguous()
        glj = None if glj is None else glj.contiguous()
        dx, dh, dtheta = flow_block_vjp(ctx.spec, ctx.integrand, x, h, fx, scaling, gz, glj, ctx.nb_steps, ctx.reverse_z,
                                        (nig[0], nig[2], any(nig[7:])), z2_saved=ctx.z2)
        ctx.z2 = None
        return (dx, None, dh, None, None, None, glj if nig[6] else None, *split_flat(dtheta, ctx.shapes, nig[7:]))


class FlowLogLikelihood(torch.autograd.Function):
    """ll[b] = sum_i log_jac[b,i] - 1/2 sum_i (log 2 pi + z[b,i]^2)  (UMNNMAFFlow.py:109-119) as one launch per direction."""

    @staticmethod
    def forward(ctx, z, log_jac):
        ll = hip_flow_ll(z, log_jac)
        ctx.save_for_backward(z.contiguous())
        return ll

    @staticmethod
    @once_differentiable
    def backward(ctx, g_ll):
        (z,) = ctx.saved_tensors
        return hip_flow_ll_backward(z, g_ll, ctx.needs_input_grad[0], ctx.needs_input_grad[1])


def fused_block_ok(x, h, scaling, x0, want_jac):
    """The one-node training path of a block applies: fp32 x-class storage (the embedding h in fp32 or bf16), lower limit 0, log_jac
    wanted, frozen scaling, no autocast."""
    return (x0 is None and want_jac and x.dtype == torch.float32 and h.dtype in (torch.float32, torch.bfloat16) and x.dim() == 2
            and not scaling.requires_grad and not torch.is_autocast_enabled() and os.environ.get("UMNN_FUSED_TRAIN", "1") != "0")


# ----------------------------------------------------------------------------------------------
# reference-shaped public API
# ----------------------------------------------------------------------------------------------
def integrate(x0, nb_steps, step_sizes, integrand, h, compute_grad=False, x_tot=None, inv_f=False,
              cc_weights=None, steps=None):
    """Clenshaw-Curtis quadrature of ``integrand`` from x0 to x0 + nb_steps*step_sizes.

    compute_grad=False -> the integral [B,d].  compute_grad=True -> (d_theta_flat, d_h) for cotangent ``x_tot``
    (what the reference's backward consumes).  ``cc_weights``/``steps`` are accepted for signature parity; the
    tables are a pure function of nb_steps and come from the per-device cache."""
    x = x0 + nb_steps * step_sizes
    spec = _hip_spec(integrand, x, multi=True)
    if compute_grad:
        if spec is None:
            return aten_backward(integrand, x0, x, h, x_tot, nb_steps, inv_f)
        with torch.no_grad():                       # (the gradients themselves are not differentiated)
            _, _, dh, dtheta = _launch_backward(_graph_mode() and spec_args(spec), spec, integrand, x0, x, h, x_tot, None, nb_steps,
                                                (False, False, True, True), inv_f)
        return dtheta, dh
    # The reference's direct integration is plain ATen, hence differentiable by ordinary autograd
    # (ParallelNeuralIntegral.py:49-65).  Keep that: only when nothing can ask for a gradient is the graph skipped.
    wants_graph = torch.is_grad_enabled() and (
        x.requires_grad or (h is not None and h.requires_grad)
        or (isinstance(integrand, torch.nn.Module) and any(p.requires_grad for p in integrand.parameters())))
    if spec is None:
        with torch.set_grad_enabled(wants_graph):
            return aten_forward(integrand, x0, x, h, nb_steps, inv_f)
    if wants_graph:
        return ParallelNeuralIntegral.apply(x0, x, integrand, _flatten(integrand.parameters()), h, nb_steps, inv_f)
    return cc_forward(spec, x0, x, h, nb_steps, inv_f)[0]


def _launch_backward(net, spec, integrand, x0, x, h, g, g_fx, nb_steps, need, inv_f=False):
    """``quadrature_backward`` -> (dx0, dx, dh, dtheta_flat), None where not needed.  ``net`` = (W[], b[], hidden_act, out_act): as the recorded
    ``umnn::cc_backward`` (which makes the same HIP / ATen choice when it runs); falsy: the eager call."""
    if not net:
        return quadrature_backward(spec, integrand, x0, x, h, g, g_fx, nb_steps, need, inv_f)
    need = [bool(need[0]) and x0 is not None, bool(need[1]), bool(need[2]), bool(need[3])]
    if net[0][-1].shape[0] == 1:
        op, cotangents = torch.ops.umnn.cc_backward, (g, g_fx)
    elif g_fx is None:
        op, cotangents = torch.ops.umnn.cc_backward_multi, (g,)
    else:
        op, cotangents = torch.ops.umnn.cc_backward_multi_fx, (g, g_fx)
    out = op(x0, x, h, *cotangents, *net, int(nb_steps), need, bool(inv_f))
    return tuple(t if n else None for t, n in zip(out, need))


def _save(ctx, spec, integrand, *tensors):
    """What a quadrature Function keeps for its backward.  Recorded (Dynamo traces both methods: they may hold nothing but tensors and
    plain values, and call nothing but torch.ops.umnn and ATen): the integrand as W[] + b[] behind ``tensors`` and its codes in
    ``ctx.net``.  Eager: the spec (None: the ATen path, decided on the calling thread -- force_generic is thread-local, backward
    runs elsewhere) and the integrand themselves."""
    if spec is not None and _graph_mode():
        W, b, ha, oa = spec_args(spec)
        ctx.net, ctx.spec, ctx.integrand = (ha, oa, len(W)), None, None
        ctx.save_for_backward(*tensors, *W, *b)
    else:
        ctx.net, ctx.spec, ctx.integrand = None, spec, integrand
        ctx.save_for_backward(*tensors)


def _saved(ctx, n):
    """-> (the n tensors of ``_save``, its ``net`` for ``_launch_backward``)."""
    saved = ctx.saved_tensors
    if ctx.net is None:
        return saved, None
    ha, oa, L = ctx.net
    return saved[:n], (list(saved[n:n + L]), list(saved[n + L:]), ha, oa)


def _quad_forward(ctx, who, x0, x, integrand, h, nb_steps, inv_f, jac):
    """forward of the quadrature operators -> (F, f_x or None).  ``jac``: the operator owns its f_x output -- True: single-output
    integrands on the HIP path only; "any": every n_out and device (``IntegralWithDerivative``)."""
    spec = _hip_spec(integrand, x, multi=jac is not True, who=who)
    if jac is True and spec is None:
        raise RuntimeError(f"{who} needs an MLP integrand on a GPU")
    ctx.nb_steps, ctx.inv_f, ctx.jac, ctx.x0_none = nb_steps, bool(inv_f), bool(jac), x0 is None      # (x0 None: lower limit 0, nothing to save)
    lims = () if x0 is None else (x0,)
    if spec is not None and _graph_mode():
        _save(ctx, spec, integrand, *lims, x, h)
    else:       # clones: callers mutate their tensors in place after the call (UMNNMAF.compute_ll clamps z, :150)
        _save(ctx, spec, integrand, *(t.clone() for t in lims), x.clone(), h)
    if spec is None:
        F = aten_forward(integrand, torch.zeros_like(x) if x0 is None else x0, x, h, nb_steps, inv_f)
        return F, (integrand(x, h) if jac else None)
    return cc_forward(spec, x0, x, h, nb_steps, inv_f)


def _quad_backward(ctx, gF, gfx, need):
    """backward of the four -> (dx0, dx, dh, dtheta_flat) for ``need``, given in that order (each class maps its own argument
    positions).  ``gfx`` is dropped for operators whose f_x output is not theirs."""
    n = 2 if ctx.x0_none else 3
    tensors, net = _saved(ctx, n)
    x0, x, h = (None if ctx.x0_none else tensors[0]), tensors[n - 2], tensors[n - 1]
    return _launch_backward(net, ctx.spec, ctx.integrand, x0, x, h, gF, gfx if ctx.jac else None, ctx.nb_steps, need, ctx.inv_f)


class ParallelNeuralIntegral(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x0, x, integrand, flat_params, h, nb_steps=20, inv_f=False):
        return _quad_forward(ctx, "ParallelNeuralIntegral", x0, x, integrand, h, nb_steps, inv_f, False)[0]

    @staticmethod
    @once_differentiable        # double backward (create_graph=True through the quadrature) raises instead of silently detaching
    def backward(ctx, grad_output):
        nig = ctx.needs_input_grad
        dx0, dx, dh, dtheta = _quad_backward(ctx, grad_output, None, (nig[0], nig[1], nig[4], nig[3]))
        return dx0, dx, None, dtheta, dh, None, None


class NeuralIntegral(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x0, x, integrand, flat_params, h, nb_steps=20):
        return _quad_forward(ctx, "NeuralIntegral", x0, x, integrand, h, nb_steps, False, False)[0]

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_output):
        nig = ctx.needs_input_grad
        dx0, dx, dh, dtheta = _quad_backward(ctx, grad_output, None, (nig[0], nig[1], nig[4], nig[3]))
        return dx0, dx, None, dtheta, dh, None


SOLVERS = {"CC": NeuralIntegral, "CCParallel": ParallelNeuralIntegral}     # the ``solver`` names of a flow block that integrate


class IntegralWithJacobian(torch.autograd.Function):
    """(F, f_x) = (int_{x0}^{x} f, f(x;h)) in one kernel pass, differentiable in both outputs.

    This is what a UMNNMAF block needs (z from F, log-det from f_x); the reference obtains f_x from a second
    integrand evaluation and a second MADE pass (UMNNMAF.py:136-139).  HIP path only."""

    @staticmethod
    def forward(ctx, x0, x, integrand, flat_params, h, nb_steps):
        return _quad_forward(ctx, "IntegralWithJacobian", x0, x, integrand, h, nb_steps, False, True)

    @staticmethod
    @once_differentiable
    def backward(ctx, gF, gfx):
        nig = ctx.needs_input_grad
        dx0, dx, dh, dtheta = _quad_backward(ctx, gF, gfx, (nig[0], nig[1], nig[4], nig[3]))
        return dx0, dx, None, dtheta, dh, None


class IntegralWithDerivative(torch.autograd.Function):
    """(F, f_x) = (int_{x0}^{x} f(t; h) dt, f(x; h)) for every integrand, n_out and device, differentiable in both outputs:

        IntegralWithDerivative.apply(x0, x, integrand, flat_params, h, nb_steps) -> (F, f_x)

    f_x is the derivative of F in its upper limit -- the density of a CDF, the hazard of a cumulative hazard -- and node 0 of the
    quadrature, so it costs no second evaluation of the integrand.  This pair is the package's replacement for
    ``torch.autograd.grad(F, x, create_graph=True)``, which raises here (every quadrature operator is ``once_differentiable``).
    A single-output MLP integrand on the GPU takes the path of ``IntegralWithJacobian`` (same kernels, same bits); an MLP integrand of
    2..16 outputs over x [B,1] on the GPU is one multi-output launch forward and the backward passes of umnn_cc_backward_multi_fx,
    which take the cotangent of f_x next to that of F; everything else -- host tensors, n_out > 16, nets beyond the LDS, arbitrary
    callables -- runs on ATen (``aten_forward`` / ``aten_vjp``).  A multi-output integrand returns [B, n_out] twice and
    dx = sum_k g_k f_k(x) + sum_k g_fx,k df_k/dx (x)."""

    @staticmethod
    def forward(ctx, x0, x, integrand, flat_params, h, nb_steps):
        return _quad_forward(ctx, "IntegralWithDerivative", x0, x, integrand, h, nb_steps, False, "any")

    @staticmethod
    @once_differentiable
    def backward(ctx, gF, gfx):
        nig = ctx.needs_input_grad
        dx0, dx, dh, dtheta = _quad_backward(ctx, gF, gfx, (nig[0], nig[1], nig[4], nig[3]))
        return dx0, dx, None, dtheta, dh, None


class IntegralWithJacobianParams(torch.autograd.Function):
    """IntegralWithJacobian with the integrand's parameters passed one by one instead of as one flat tensor: no
    ``torch.cat`` in the forward and no cat-backward (a narrow + copy per parameter) in the backward -- the gradients are
    views into the kernel's flat d_theta.  Internal to the flow blocks; the public operators keep the reference's
    ``flat_params`` signature."""

    @staticmethod
    def forward(ctx, x0, x, integrand, h, nb_steps, *params):
        ctx.shapes = [p.shape for p in params]
        return _quad_forward(ctx, "IntegralWithJacobianParams", x0, x, integrand, h, nb_steps, False, True)

    @staticmethod
    @once_differentiable
    def backward(ctx, gF, gfx):
        nig = ctx.needs_input_grad
        dx0, dx, dh, dtheta = _quad_backward(ctx, gF, gfx, (nig[0], nig[1], nig[3], any(nig[5:])))
        return (dx0, dx, None, dh, None, *split_flat(dtheta, ctx.shapes, nig[5:]))


class InverseNeuralIntegral(torch.autograd.Function):
    """x [B,d] with int_0^x f(s; h) ds = t: the inverse of ``ParallelNeuralIntegral.apply(0, x, ...)`` in x, by the safeguarded
    Newton iteration of ``umnn_cc_solve`` (one launch per dimension on the HIP path; ``newton_solve`` on ATen otherwise).

        InverseNeuralIntegral.apply(t, integrand, flat_params, h, nb_steps=20, x_range=(-50., 50.), tol=1e-6, max_iter=64,
                                    return_info=False)  ->  x   or   (x, f(x), status)

    The gradient is the implicit one: dx/dt = 1 / f(x), and (d_theta, d_h) are those of the forward integral with upper limit x for
    the cotangent -g_x / f(x) -- one launch of the existing backward kernels, no backward kernel of its own."""

    @staticmethod
    def forward(ctx, t, integrand, flat_params, h, nb_steps=20, x_range=(-50., 50.), tol=1e-6, max_iter=64, return_info=False):
        lo, hi = float(x_range[0]), float(x_range[1])
        spec = _hip_spec(integrand, t, who="InverseNeuralIntegral")
        if spec is None:
            x, fx, status = aten_solve(integrand, h.detach(), t.detach(), nb_steps, lo, hi, tol, max_iter)
        elif _graph_mode():
            x, fx, status = torch.ops.umnn.cc_solve(t, h, *spec_args(spec), int(nb_steps), lo, hi, float(tol), int(max_iter))
        else:
            x, fx, status = solve_integral(spec, t, h, nb_steps, lo, hi, tol, max_iter)
        ctx.nb_steps = nb_steps
        _save(ctx, spec, integrand, x, h, fx)
        if not return_info:
            return x
        ctx.mark_non_differentiable(fx, status)
        return x, fx, status

    @staticmethod
    @once_differentiable
    def backward(ctx, g_x, *_unused):
        nig = ctx.needs_input_grad
        (x, h, fx), net = _saved(ctx, 3)
        g_t = g_x / fx
        dh = dtheta = None
        if nig[2] or nig[3]:
            _, _, dh, dtheta = _launch_backward(net, ctx.spec, ctx.integrand, None, x, h, -g_t, None, ctx.nb_steps,
                                                (False, False, nig[3], nig[2]))
        return (g_t if nig[0] else None, None, dtheta, dh, None, None, None, None, None)


class InverseIntegralSum(torch.autograd.Function):
    """x [B,1] with sum_k coef[b,k] int_0^x f_k(s; h_b) ds = t[b]: the inverse, in x, of a non-negative combination of the K curves
    of a multi-output integrand -- the event time of K competing risks (sum_k H_k(T) = -log U), a quantile of a mixture of K CDFs.

        InverseIntegralSum.apply(t, coef, integrand, flat_params, h, nb_steps=20, x_range=(-50., 50.), tol=1e-6, max_iter=64,
                                 return_info=False)  ->  x [B,1]   or   (x, f [B,K], status [B,1])

    t [B,1], coef [B,K] with coef >= 0 and a positive entry per row (not checked: a check would synchronise; a row of zeros follows
    the clamping rule).  On GPU tensors an MLP integrand of 2..16 outputs is ONE launch of umnn_cc_solve_multi (the safeguarded
    Newton iteration of umnn_cc_solve on the K-output quadrature, exact fp32); everything else runs ``newton_solve_sum``.  f is
    f_k(x; h) at the returned x (cause probabilities are proportional to coef_k f_k), status the word of ``InverseNeuralIntegral``.

    Once-differentiable by the implicit-function theorem, from what the forward saved and one existing backward: with
    D = sum_k coef_k f_k(x),  g_t = g_x / D,  g_coef = -g_t F_k(x),  and (d_theta, d_h) those of the K integrals up to x for the
    cotangent -g_t coef [B,K] (the multi-output backward).  No special case for clamped rows, as in ``InverseNeuralIntegral``."""

    @staticmethod
    def forward(ctx, t, coef, integrand, flat_params, h, nb_steps=20, x_range=(-50., 50.), tol=1e-6, max_iter=64, return_info=False):
        lo, hi = float(x_range[0]), float(x_range[1])
        if coef.dim() != 2 or coef.shape[0] != t.shape[0] or coef.shape[1] < 2:
            raise RuntimeError(f"umnn_amd: InverseIntegralSum takes coef [B, K] with K >= 2 next to t [B, 1]; got {tuple(coef.shape)} "
                               f"and {tuple(t.shape)} (one curve: InverseNeuralIntegral on t / coef)")
        spec = _hip_spec(integrand, t, multi=True, who="InverseIntegralSum")
        if spec is not None and _graph_mode():
            x, F, fx, status = torch.ops.umnn.cc_solve_multi(t, coef, h, *spec_args(spec), int(nb_steps), lo, hi, float(tol), int(max_iter))
        else:
            x, F, fx, status = solve_sum(spec, integrand, t, coef, h, nb_steps, lo, hi, tol, max_iter)
        ctx.nb_steps = nb_steps
        _save(ctx, spec, integrand, x, h, coef, F, fx)
        if not return_info:
            return x
        ctx.mark_non_differentiable(fx, status)
        return x, fx, status

    @staticmethod
    @once_differentiable
    def backward(ctx, g_x, *_unused):
        nig = ctx.needs_input_grad
        (x, h, coef, F, fx), net = _saved(ctx, 5)
        g_t = g_x / (coef * fx).sum(1, keepdim=True)
        dh = dtheta = None
        if nig[3] or nig[4]:
            _, _, dh, dtheta = _launch_backward(net, ctx.spec, ctx.integrand, None, x, h, -g_t * coef, None, ctx.nb_steps,
                                                (False, False, nig[4], nig[3]))
        return (g_t if nig[0] else None, -g_t * F if nig[1] else None, None, dtheta, dh, None, None, None, None, None)
