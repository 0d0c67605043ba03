"""MADE conditioner (adjacent row a13 of the scope table): produces the embedding h the quadrature consumes.

Mirrors models/UMNN/made.py (MaskedLinear :16-27, MADE :30-144, ConditionnalMADE :146-195): constructor
signatures, ``net.{0,2,..}.{weight,bias,mask}`` state_dict keys and mask construction are the reference's.  The
GEMMs stay on PyTorch-ROCm (hipBLASLt): at the BSDS300 shape they are ~2 % of a block's FLOPs.
MI355X-side changes that do not alter results: the masked weight ``mask*W`` is cached between calls while the
weight is unchanged and no graph is being recorded, and ConditionnalMADE only computes the output columns it keeps.

Inference fast path (CUDA tensors, autograd off, env ``UMNN_MADE_BF16X3`` != 0): every masked linear runs as ONE bf16
GEMM with fp32 accumulation, ``[xh | xl | xh | 1 | 1] @ [Wh | Wh | Wl | bh | bl]^T`` (x = xh + xl, W = Wh + Wl in bf16
pieces): the fp32 hipBLASLt GEMM of the BSDS300 output layer takes 168 us, this one 60 us, max error 3e-6 of the output
range.  The left operand is built by the HIP kernel ``umnn_made_split3`` (csrc/made_split.hip) straight from the
previous layer's raw output (ReLU fused); the packed weights are cached like the masked weight.  Training (autograd on)
keeps the fp32 ``F.linear`` chain.

How a call is routed is decided in one place, ``conditioner_route`` (the table is in DESIGN.md, "Conditioner routes"), executed by
``_run_route``; what may be cached is decided in one place, ``MaskedLinear._cached``; the switches are one record, ``_OPTIONS``.
"""
import collections
import ctypes
import dataclasses
import math
import os
import threading
import warnings

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

from ._common import _graph_mode, _stream, _address as _ptr

_capture_state = threading.local()      # .cache_ok: a capture on THIS thread that tracks weight versions itself (GraphedLL)


class capture_may_cache:
    """Context manager (graphs.GraphedLL): the hipGraph being captured on this thread re-captures when a weight version
    moves, so the conditioner's cached masked / packed weights may be baked into it."""

    def __enter__(self):
        self._old = getattr(_capture_state, "cache_ok", False)
        _capture_state.cache_ok = True

    def __exit__(self, *exc):
        _capture_state.cache_ok = self._old


class MaskedLinear(nn.Linear):
    """nn.Linear whose weight is multiplied elementwise by a fixed 0/1 ``mask`` buffer."""

    def __init__(self, in_features, out_features, bias=True):
        super().__init__(in_features, out_features, bias)
        self.register_buffer('mask', torch.ones(out_features, in_features))
        self._slots = {}        # slot -> (key, value) of _cached: "masked", "packed", "frags"; on a MADE's first layer also its "plan"
        self._epoch = 0         # bumped by set_mask / invalidate_caches: part of the key of MADE.progressive_plan

    def set_mask(self, mask):
        # mask arrives [in, out] (numpy, bool); stored [out, in] like the weight
        self.mask.data.copy_(torch.from_numpy(np.ascontiguousarray(mask.T).astype(np.float32)))
        self.invalidate_caches()

    def invalidate_caches(self):
        """Drop the cached masked / packed weights.  The caches are keyed on tensor versions; writes through ``.data``
        (or any other route that does not bump ``_version``) are invisible to that key, so code doing such writes must
        call this (``umnn_amd.invalidate_caches(model)`` does it for a whole model)."""
        self._slots = {}
        self._epoch += 1

    @staticmethod
    def _may_store(t):
        """Nothing produced while a stream capture is recording may enter a cache: its kernels have only been recorded, the tensor
        holds nothing until that graph is replayed, and an eager call (or a second capture) that found it under a matching key
        would read uninitialised weights.  (A capture that may bake the caches -- graphs.GraphedLL -- fills them with an eager
        run BEFORE it records; a miss inside the capture is then recomputed inside the graph, which is merely slower.)"""
        return not (t.is_cuda and torch.cuda.is_current_stream_capturing())

    def _cached(self, slot, key, build):
        """The one cache rule: ``build()`` under ``slot`` while ``key`` (tensor versions and pointers) is unchanged.
          * a hit on an equal key returns the stored object;
          * inside a hipGraph capture the value must be part of the graph -- a cached tensor would be baked in as a constant and
            replays after an optimizer step would read stale conditioner weights -- so it is built and not looked up, unless the
            capture tracks the weights' versions itself (``capture_may_cache``: graphs.GraphedLL re-captures when they move);
          * nothing built while a stream is capturing is ever stored (``_may_store``)."""
        may_store = self._may_store(self.weight)
        if may_store or getattr(_capture_state, "cache_ok", False):
            hit = self._slots.get(slot)
            if hit is not None and hit[0] == key:
                return hit[1]
        value = build()
        if may_store:
            self._slots[slot] = (key, value)
        return value

    def _weight_key(self):
        return (self.weight._version, self.weight.data_ptr(), self.mask._version, self.mask.data_ptr())

    def _key(self, rows=None):
        return self._weight_key() + (self.bias._version, self.bias.data_ptr(), None if rows is None else rows.data_ptr())

    def _masked(self, rows):
        """(mask * weight, bias), or their ``rows`` only."""
        W, b = self.mask * self.weight, self.bias
        return (W, b) if rows is None else (W.index_select(0, rows), b.index_select(0, rows))

    def masked_weight(self):
        if torch.is_grad_enabled() and self.weight.requires_grad:
            return self.mask * self.weight
        return self._cached("masked", self._weight_key(), lambda: (self.mask * self.weight).detach())

    def packed_bf16(self, rows=None):
        """[Wh | Wh | Wl | bh | bl | 0-pad] as bf16 [N, pad8(3K+2)] for the K-concatenated bf16 GEMM (cached while
        weight, mask and bias are unchanged).  ``rows``: optional output-row selection (ConditionnalMADE)."""
        def build():
            with torch.no_grad():
                W, b = self._masked(rows)
                Wh, bh = W.bfloat16(), b.bfloat16()
                Wl, bl = (W - Wh.float()).bfloat16(), (b - bh.float()).bfloat16()
                pad = (-(3 * W.shape[1] + 2)) % 8
                return torch.cat([Wh, Wh, Wl, bh[:, None], bl[:, None],
                                  torch.zeros(W.shape[0], pad, dtype=torch.bfloat16, device=W.device)], 1).contiguous()
        return self._cached("packed", self._key(rows), build)

    def packed_fragments(self, rows=None):
        """(fragments, bias) for ``umnn_made_mlp_forward``: the masked weight as bf16 MFMA fragments
        [tile][K-step][piece hi/lo][lane][8] in the K order of include/umnn_cc.h, and the fp32 bias (cached while weight, mask
        and bias are unchanged).  ``rows``: optional output-row selection (ConditionnalMADE)."""
        def build():
            with torch.no_grad():
                W, b = self._masked(rows)
                return pack_fragments(W.float()), b.float().contiguous()
        return self._cached("frags", self._key(rows), build)

    def forward(self, input):
        if _graph_mode():           # the reference's composition (made.py:26-27): no cache keyed on versions or pointers
            return F.linear(input, self.mask * self.weight, self.bias)
        return F.linear(input, self.masked_weight(), self.bias)


_FRAG_INDEX = {}      # (N, K, device) -> gather indices of pack_fragments


def pack_fragments(W):
    """[N, K] fp32 -> bf16 [T, S, 2, 64, 8]: A-operand fragments of v_mfma_f32_16x16x32_bf16 for D[out][row] = W[out][k] act[k][row].
    Lane (g = lane >> 4, rho = lane & 15) of fragment (tile t, K-step s) holds, in slot j, W[16t + rho][32s + 16(j>>2) + 4g + (j&3)]
    (zero outside the matrix) -- the K order in which the fused kernel's accumulators are the next layer's operand; piece 0 is
    the value rounded to bf16, piece 1 the rounded remainder."""
    N, K = W.shape
    T, S = (N + 15) // 16, (K + 31) // 32
    key = (N, K, W.device)
    idx = _FRAG_INDEX.get(key)
    if idx is None:
        lane = torch.arange(64, device=W.device)
        g, rho = lane >> 4, lane & 15
        j = torch.arange(8, device=W.device)
        n = 16 * torch.arange(T, device=W.device).view(T, 1, 1, 1) + rho.view(1, 1, 64, 1)                       # [T,1,64,1]
        k = 32 * torch.arange(S, device=W.device).view(1, S, 1, 1) + (16 * (j >> 2) + (j & 3)).view(1, 1, 1, 8) \
            + 4 * g.view(1, 1, 64, 1)                                                                            # [1,S,64,8]
        idx = (n.expand(T, S, 64, 8) * (32 * S) + k.expand(T, S, 64, 8)).reshape(-1)
        if MaskedLinear._may_store(W):      # (indices built inside a capture would make an eager call gather with garbage)
            if len(_FRAG_INDEX) > 64:
                _FRAG_INDEX.clear()
            _FRAG_INDEX[key] = idx
    Wp = torch.zeros(16 * T, 32 * S, dtype=torch.float32, device=W.device)
    Wp[:N, :K] = W
    frag = Wp.reshape(-1).index_select(0, idx).view(T, S, 64, 8)
    hi = frag.bfloat16()
    lo = (frag - hi.float()).bfloat16()
    return torch.stack((hi, lo), 2).contiguous()


def invalidate_caches(module):
    """Drop every MaskedLinear cache under ``module`` (after writes that bypass tensor versioning, e.g. ``p.data``)."""
    for m in module.modules():
        if isinstance(m, MaskedLinear):
            m.invalidate_caches()


# ---- the switches ----------------------------------------------------------------------------------------------------------------
@dataclasses.dataclass
class MadeOptions:
    """Every switch of the conditioner, read from the environment once at import (``_OPTIONS``); ``set_made_fast_path`` and
    ``set_made_fused`` change the first six at run time.  (``UMNN_MADE_LINEAR_RT`` / ``_G``, the tuning knobs of made_linear_kernel,
    are read per call: tools/made_layered_check.py changes them at run time.)"""
    fast: bool                      # UMNN_MADE_BF16X3 != 0: the inference fast path
    fused: bool                     # UMNN_MADE_FUSED != 0: the conditioner kernels (one launch, hidden stack, one per layer)
    max_rows: int                   # UMNN_MADE_FUSED_MAX_ROWS: the batch size up to which they are used
    wide_out: bool                  # UMNN_MADE_FUSED_WIDE_OUT == 1: outputs wider than 512 in the one-launch kernel too
    hybrid: bool                    # UMNN_MADE_FUSED_HYBRID == 1: wide outputs as hidden stack in the kernel + one library GEMM
    layered: bool                   # UMNN_MADE_LAYERED != 0: wide outputs as one made_linear_kernel launch per masked linear
    layered_max_rows: int           # UMNN_MADE_LAYERED_MAX_ROWS: ... up to this many rows
    # above this many rows a wide OUTPUT layer goes back to split + library GEMM (hipBLASLt's large tiles win there: 67 + 9 us against
    # 97 us at 8192 x 512 x 1890), the hidden layers stay on made_linear_kernel (11-13 us against 9 + 23 us each)
    layered_lib_out_rows: int       # UMNN_MADE_LAYERED_LIB_OUT_ROWS
    train_fused: bool               # UMNN_MADE_TRAIN_FUSED != 0: the training chain as one autograd node
    addmm_act: bool                 # UMNN_MADE_ADDMM_ACT != 0 and torch has _addmm_activation: bias + ReLU in the GEMM epilogue
    probe: object = None            # None until _probe ran: whether torch.mm(bf16, bf16, out_dtype=float32) works here


def _options_from_env(env):
    return MadeOptions(fast=env.get("UMNN_MADE_BF16X3", "1") != "0", fused=env.get("UMNN_MADE_FUSED", "1") != "0",
                       max_rows=int(env.get("UMNN_MADE_FUSED_MAX_ROWS", "32768")), wide_out=env.get("UMNN_MADE_FUSED_WIDE_OUT", "0") == "1",
                       hybrid=env.get("UMNN_MADE_FUSED_HYBRID", "0") == "1", layered=env.get("UMNN_MADE_LAYERED", "1") != "0",
                       layered_max_rows=int(env.get("UMNN_MADE_LAYERED_MAX_ROWS", "32768")),
                       layered_lib_out_rows=int(env.get("UMNN_MADE_LAYERED_LIB_OUT_ROWS", "4096")),
                       train_fused=env.get("UMNN_MADE_TRAIN_FUSED", "1") != "0",
                       addmm_act=hasattr(torch, "_addmm_activation") and env.get("UMNN_MADE_ADDMM_ACT", "1") != "0")


_OPTIONS = _options_from_env(os.environ)


class _Switch:
    """One field of ``_OPTIONS`` under its earlier spelling ``NAME["enabled"]`` (tests/test_gpu_round6.py sets ``_TRAIN_FUSED`` so)."""

    def __init__(self, field):
        self.field = field

    def __getitem__(self, key):
        return getattr(_OPTIONS, self.field)

    def __setitem__(self, key, value):
        setattr(_OPTIONS, self.field, bool(value))


_TRAIN_FUSED = _Switch("train_fused")


def set_made_fast_path(enabled):
    """Inference conditioner GEMMs as K-concatenated bf16 GEMMs (True, default) or plain fp32 ``F.linear`` (False)."""
    _OPTIONS.fast = bool(enabled)


def get_made_fast_path():
    return _OPTIONS.fast


def set_made_fused(enabled, max_rows=None, wide_out=None, hybrid=None, layered=None):
    """The whole conditioner of a block as ONE launch (``umnn_made_mlp_forward``) on the inference path when every width is
    <= 512 (see ``conditioner_route``) and the batch has at most ``max_rows`` rows (default 32768).  ``False``: always the per-layer
    path.  ``wide_out=True`` lifts the limit on the OUTPUT width (tests / measurements)."""
    _OPTIONS.fused = bool(enabled)
    if max_rows is not None:
        _OPTIONS.max_rows = int(max_rows)
    if wide_out is not None:
        _OPTIONS.wide_out = bool(wide_out)
    if hybrid is not None:           # wide outputs: hidden stack in the kernel, output layer as one library GEMM (measured: no gain)
        _OPTIONS.hybrid = bool(hybrid)
    if layered is not None:          # wide outputs: one launch of the kernel per masked linear, grid over rows x output tiles
        _OPTIONS.layered = bool(layered)


def _probe(cuda_fp32, device):
    """The lazy probe of the bf16x3 GEMM path, run once and only where that path could be taken (CUDA fp32 input, autograd off, the
    switch on): HIP library present, torch.mm(out_dtype=) available."""
    if torch.is_grad_enabled() or not cuda_fp32 or not _OPTIONS.fast:
        return False
    if _OPTIONS.probe is None:
        from . import _lib
        _lib.lib()              # a missing HIP library is an error on a GPU box (HipLibraryMissing), never a silent fallback
        try:
            a = torch.zeros(8, 8, dtype=torch.bfloat16, device=device)
            torch.mm(a, a.t(), out_dtype=torch.float32)
            _OPTIONS.probe = True
        except (TypeError, RuntimeError, NotImplementedError) as e:     # a torch build without mm(out_dtype=) on this device
            _OPTIONS.probe = False
            warnings.warn("umnn_amd: torch.mm(bf16, bf16, out_dtype=float32) is not available here "
                          f"({type(e).__name__}: {e}); the inference conditioner runs the fp32 F.linear chain instead of the "
                          "K-concatenated bf16 GEMMs.", RuntimeWarning, stacklevel=4)
    return _OPTIONS.probe


def _fast_path_ok(x):
    """bf16x3 GEMM path: CUDA fp32 input, autograd off, HIP library present, torch.mm(out_dtype=) available."""
    return _probe(x.is_cuda and x.dtype == torch.float32, x.device)


# ---- the route -------------------------------------------------------------------------------------------------------------------
Route = collections.namedtuple("Route", "name no_cat lib_out")
Route.__doc__ = """What one conditioner call does.  ``name``: "graph" | "split" | "fused" | "hybrid" | "layered" | "train" | "linear"
(the rows of DESIGN.md's route table); ``no_cat``: ConditionnalMADE's two input blocks are read without the cat; ``lib_out``
("layered" only): the output layer goes to split + library GEMM."""
_FAST_ROUTES = ("split", "fused", "hybrid", "layered")


def conditioner_route(rows, widths, n_out, cuda_fp32, two_fp32_blocks, grad, needs_grad, autocast, graph, probe, opts):
    """The only route decision: a function of values (no library load, no probe, no device call) -> ``Route``.
      rows: batch rows; widths: (in_features, out_features) per masked linear; n_out: the output width that survives;
      cuda_fp32: the chain's input (after ``_to_weight_dtype``) is a CUDA fp32 tensor; two_fp32_blocks: it arrives as two fp32 column
      blocks on fp32 weights; grad: grad mode; needs_grad: a 2-D input on CUDA fp32 weights with biases of which something requires
      grad; autocast; graph: ``_graph_mode()``; probe: the result of ``_probe``; opts: a ``MadeOptions``."""
    if graph:                                   # torch.compile / export / jit.trace: the reference's fp32 F.linear chain
        return Route("graph", False, False)
    if not grad and cuda_fp32 and opts.fast and probe:
        if not opts.fused or rows > opts.max_rows or len(widths) > 8 or any(k > 512 for k, _ in widths):
            return Route("split", False, False)
        if n_out <= 512 or opts.wide_out:
            return Route("fused", False, False)
        if len(widths) >= 2 and opts.hybrid:
            return Route("hybrid", False, False)
        if opts.layered and rows <= opts.layered_max_rows:
            return Route("layered", two_fp32_blocks, len(widths) > 1 and rows > opts.layered_lib_out_rows and widths[-1][1] > 512)
        return Route("split", False, False)
    if opts.train_fused and grad and cuda_fp32 and not autocast and needs_grad:
        return Route("train", False, False)
    return Route("linear", False, False)


def _split_gemm(lib, stream, raw, relu, packed, bf16, fill=None):
    """One masked linear as the K-concatenated bf16 GEMM on ``packed`` [N, pad8(3K+2)]: the left operand [xh | xl | xh | 1 | 1] is
    written by one ``umnn_made_split3`` launch from ``raw`` (ReLU fused if ``relu``) or by ``fill(op)``; the GEMM accumulates in fp32
    and writes fp32, or bf16 (configuration C4: the [B, E*d] embedding the quadrature kernels then read with bf16 loads)."""
    from . import _lib
    op = torch.empty(raw.shape[0], packed.shape[1], dtype=torch.bfloat16, device=raw.device)
    if fill is None:
        _lib.check(lib.umnn_made_split3(_ptr(raw), raw.shape[0], raw.shape[1], 1 if relu else 0, _ptr(op), op.shape[1], stream),
                   "made_split3")
    else:
        fill(op)
    return torch.mm(op, packed.t()) if bf16 else torch.mm(op, packed.t(), out_dtype=torch.float32)


def _run_route(route, a, a2, layers, keep, out_dtype, select=None):
    """Execute ``route`` on a [B, K0] (or its two column blocks a | a2) through the MaskedLinear / ReLU chain ``layers``; ``keep``: the
    rows of the last layer that are computed (ConditionnalMADE), ``select``: rows taken from its cached FULL packed weight
    (``raw_rows``).  The fast routes write ``out_dtype`` = bf16 themselves; the others return the chain's dtype.
      "split":   per layer one split launch + one library GEMM;
      "fused":   the whole MLP in one launch of the fused kernel (csrc/made_fused.hip);
      "hybrid":  its hidden stack in one launch, whose last ReLU output leaves as the bf16 operand of the output layer's library GEMM;
      "layered": one launch of ``made_linear_kernel`` per masked linear (``umnn_made_linear_forward``: grid over row groups x
                 output-tile groups, the bf16 split and the previous layer's ReLU in the operand load, ConditionnalMADE's two blocks
                 read without the cat), the output layer as in "split" if ``route.lib_out``;
      "train":   the one-node training chain; "graph" / "linear": masked ``F.linear`` + ReLU."""
    name = route.name
    if name == "train":
        return _train_chain(a, layers, keep)
    if name not in _FAST_ROUTES:
        for layer in layers[:-1]:
            a = torch.relu(layer(a))
        if keep is None:
            return layers[-1](a)
        return F.linear(a, layers[-1].masked_weight().index_select(0, keep), layers[-1].bias.index_select(0, keep))
    from . import _lib
    lib = _lib.lib()
    bf16 = out_dtype == torch.bfloat16
    cur, cur2 = a.contiguous(), (None if a2 is None else a2.contiguous())
    B, dev = cur.shape[0], a.device
    with torch.cuda.device(dev):
        stream = _stream(dev)
        if name in ("fused", "hybrid"):
            inner = layers if name == "fused" else layers[:-1]
            net, held = _lib.MadeNet(), []
            net.n_layers = len(inner)
            net.widths[0] = inner[0].in_features
            for i, layer in enumerate(inner):
                frags, bias = layer.packed_fragments(keep if layer is layers[-1] else None)
                held += [frags, bias]
                net.widths[i + 1] = bias.shape[0]
                net.W[i], net.b[i] = _ptr(frags), _ptr(bias)

            def launch(out, mode, ld=0):
                _lib.check(lib.umnn_made_mlp_forward_ex(ctypes.byref(net), _ptr(cur), B, _ptr(out), mode, ld, stream), "umnn_made_mlp_forward")
            if name == "hybrid":
                return _split_gemm(lib, stream, cur, True, layers[-1].packed_bf16(keep), bf16, fill=lambda op: launch(op, 2, op.shape[1]))
            out = torch.empty(B, net.widths[len(inner)], device=dev, dtype=torch.bfloat16 if bf16 else torch.float32)
            launch(out, 1 if bf16 else 0)
            return out
        # (made_linear_kernel's tuning knobs, read per call: tools/made_layered_check.py changes them at run time)
        rt, fg = (int(os.environ.get("UMNN_MADE_LINEAR_RT", "0")), int(os.environ.get("UMNN_MADE_LINEAR_G", "0"))) if name == "layered" else (0, 0)
        for i, layer in enumerate(layers):
            last = i == len(layers) - 1
            if name == "split" or (last and route.lib_out):
                packed = layer.packed_bf16(keep if last else None)
                if last and select is not None:         # (from the cached full weight: a per-call selection never enters the layer's cache)
                    packed = packed.index_select(0, select)
                cur = _split_gemm(lib, stream, cur, i > 0, packed, last and bf16)
                continue
            frags, bias = layer.packed_fragments(keep if last else None)
            out = torch.empty(B, bias.shape[0], device=dev, dtype=torch.bfloat16 if last and bf16 else torch.float32)
            K = cur.shape[1] + (0 if cur2 is None else cur2.shape[1])
            _lib.check(lib.umnn_made_linear_forward(_ptr(frags), _ptr(bias), K, bias.shape[0], _ptr(cur),
                                                    None if cur2 is None else _ptr(cur2), cur.shape[1], B, 1 if i > 0 else 0,
                                                    _ptr(out), 1 if last and bf16 else 0, rt, fg, stream), "umnn_made_linear_forward")
            cur, cur2 = out, None
    return cur


# ---- training chain (round 6): the whole masked MLP as ONE autograd node ---------------------------------------------------------
# Under autograd the reference's chain (made.py:16-27,113-119) is, per masked linear, a mask product + F.linear + ReLU forward and a
# ReluBackward pass, two GEMMs, a column reduction for the bias gradient and the mask product's own backward: at the UCI shapes 15
# bias reductions of 16 us, 30 mask products and 20 ReLU passes per training step.  Here the chain is one node: the forward
# runs the same fp32 library GEMMs on the cached masked weight (one product per optimizer step, no autograd node), the ReLU in place;
# the backward runs, per layer, ONE pass that applies the ReLU mask to the incoming gradient and reduces the bias gradient in a fixed
# order (umnn_made_relu_bwd_bias: data-parallel replicas stay bit-identical), the two GEMMs, and the mask on the weight gradient in place.
class _MadeTrainChain(torch.autograd.Function):
    """out = MaskedLinear_L(ReLU(... ReLU(MaskedLinear_1(a)))) [rows ``keep`` of the last layer only] as one node.
    apply(a, layers, keep, W_1, b_1, ..., W_L, b_L): ``layers`` the MaskedLinear modules (for their masks / cached masked weights),
    the parameters passed as tensors so that autograd routes their gradients."""

    @staticmethod
    def forward(ctx, a, layers, keep, *params):
        acts, weffs = [a.contiguous()], []
        cur = acts[0]
        for i, layer in enumerate(layers):
            last = i == len(layers) - 1
            W, b = layer.masked_weight(), layer.bias.detach()        # (grad mode is off in here: the cached product, no autograd node)
            if last and keep is not None:
                W, b = W.index_select(0, keep), b.index_select(0, keep)
            weffs.append(W)
            if not last:
                # bias + ReLU in the GEMM's epilogue (hipBLASLt): no separate activation pass over [B, N]
                cur = y = torch._addmm_activation(b, cur, W.t(), use_gelu=False) if _OPTIONS.addmm_act else torch.relu_(torch.addmm(b, cur, W.t()))
                acts.append(cur)
            else:
                y = torch.addmm(b, cur, W.t())
        ctx.layers, ctx.keep, ctx.n = layers, keep, len(layers)
        ctx.save_for_backward(*acts, *weffs)
        return y

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g):
        from . import _lib
        lib = _lib.lib()
        L = ctx.n
        acts, weffs = ctx.saved_tensors[:L], ctx.saved_tensors[L:]
        layers, keep = ctx.layers, ctx.keep
        g = g.contiguous()
        B = g.shape[0]
        grads = [None] * (2 * L)
        stream = _stream(g.device)
        with torch.cuda.device(g.device):
            for i in range(L - 1, -1, -1):
                last = i == L - 1
                layer = layers[i]
                N = g.shape[1]
                relu_out = None if last else acts[i + 1]
                need_b = ctx.needs_input_grad[3 + 2 * i + 1]
                if need_b or not last:
                    rb = int(lib.umnn_made_relu_bwd_bias_row_blocks(B, N))
                    partial = torch.empty(rb * N, device=g.device, dtype=torch.float32)
                    gb = torch.empty(N, device=g.device, dtype=torch.float32)
                    _lib.check(lib.umnn_made_relu_bwd_bias(_ptr(g), None if relu_out is None else _ptr(relu_out), B, N,
                                                           _ptr(partial), rb, _ptr(gb), stream), "umnn_made_relu_bwd_bias")
                    if need_b:
                        if last and keep is not None:
                            full = torch.zeros_like(layer.bias)
                            full.index_copy_(0, keep, gb)
                            gb = full
                        grads[2 * i + 1] = gb
                if ctx.needs_input_grad[3 + 2 * i]:
                    gW = torch.mm(g.t(), acts[i])
                    if last and keep is not None:
                        full = torch.zeros_like(layer.weight)
                        full.index_copy_(0, keep, gW.mul_(layer.mask.index_select(0, keep)))
                        gW = full
                    else:
                        gW.mul_(layer.mask)
                    grads[2 * i] = gW
                if i > 0 or ctx.needs_input_grad[0]:
                    g = torch.mm(g, weffs[i])
        return (g if ctx.needs_input_grad[0] else None, None, None, *grads)


def _train_chain(a, layers, keep=None):
    params = []
    for l in layers:
        params += [l.weight, l.bias]
    return _MadeTrainChain.apply(a, layers, keep, *params)


def _to_weight_dtype(x, layer):
    """bf16 / fp16 activations handed to fp32 weights outside autocast: widen (exact) instead of failing in F.linear."""
    if x.dtype != layer.weight.dtype and not torch.is_autocast_enabled():
        return x.to(layer.weight.dtype)
    return x


def _cast(out, out_dtype):
    return out.to(out_dtype) if out_dtype is not None and out.dtype != out_dtype else out


class ProgressivePlan:
    """What ``MADE.progressive_plan`` returns: every hidden layer sorted by degree (stable), the masked weights permuted into that
    order, the output layer regrouped by flow dimension and the per-step table (see ``MADE.progressive_plan``).
      c, d, E, widths [H_l], ldk [K stride of W[l], a multiple of 4], orders [int64 device index per hidden layer],
      steps  int32 numpy [d][L + 1][3]: (first new unit, end of new units, input prefix length) per step and layer,
      W[l] [H_l, ldk[l]] / b[l] [H_l] for l < L; W[L] [d, E, ldk[L]] / b[L] [d, E]  (the weights' dtype, K axis zero-padded),
      max_new: the widest new-unit slice of one step, desc: the ``umnn_made_plan`` of ``umnn_made_step`` (None where the kernel does
      not apply: host tensors, non-fp32 weights, more layers or a wider slice than it holds)."""

    def __init__(self, static, W, b):
        self.__dict__.update(static)
        self.W, self.b = W, b
        self.desc = None
        dev = W[0].device
        if (dev.type == "cuda" and W[0].dtype == torch.float32 and len(self.widths) <= 8 and self.max_new <= 479):
            from . import _lib
            desc = _lib.MadePlan()
            desc.n_hidden, desc.d, desc.c, desc.E = len(self.widths), self.d, self.c, self.E
            for l, w in enumerate(self.widths):
                desc.width[l] = w
            for l in range(len(self.widths) + 1):
                desc.ldk[l] = self.ldk[l]
                desc.W[l], desc.b[l] = _ptr(W[l]), _ptr(b[l])
            desc.steps = self.steps.ctypes.data
            self.desc = desc

    def walk(self, x, context, use_kernel):
        return ProgressiveWalk(self, x, context, use_kernel)

    # (the descriptor holds raw pointers: a copied or pickled module rebuilds its plan on first use)
    def __deepcopy__(self, memo):
        return None

    def __reduce__(self):
        return (type(None), ())


class ProgressiveWalk:
    """The standing state of one block's progressive walk over ``x`` [B, d] (filled in place by the caller, column j final before
    ``step(j + 1)``): the activation buffers of the hidden layers in degree order and the embedding buffer h [B, E*d].
    ``step(j)`` computes the units that became ready and the E outputs of dimension j -> h (columns e*d + j written).
    ``use_kernel``: one ``umnn_made_step`` launch per step; otherwise the same walk as ``F.linear`` on the slices."""

    def __init__(self, plan, x, context, use_kernel):
        self.plan, self.x = plan, x
        B, dev = x.shape[0], x.device
        self.kernel = bool(use_kernel and plan.desc is not None and B > 0)
        dt = torch.float32 if self.kernel else plan.W[0].dtype
        if context is not None and (context.dtype != dt or not context.is_contiguous()):
            context = context.to(dt).contiguous()
        self.context = context
        self.row_tiles = 0          # umnn_made_step's row_tiles (0: automatic); the result does not depend on it
        L = len(plan.widths)
        self.acts = [torch.zeros(B, plan.ldk[l + 1], device=dev, dtype=dt) for l in range(L)]
        self.h = torch.zeros(B, plan.E * plan.d, device=dev, dtype=dt)
        if self.kernel:
            self._act_ptrs = (ctypes.c_void_p * 8)(*[_ptr(a) for a in self.acts])

    def step(self, j):
        p = self.plan
        B = self.x.shape[0]
        if self.kernel:
            from . import _lib
            with torch.cuda.device(self.x.device):
                _lib.check(_lib.lib().umnn_made_step(ctypes.byref(p.desc), int(j), None if self.context is None else _ptr(self.context),
                                                     _ptr(self.x), self._act_ptrs, _ptr(self.h), B, int(self.row_tiles),
                                                     _stream(self.x.device)),
                           "umnn_made_step")
            return self.h
        L = len(p.widths)
        dt = p.W[0].dtype
        for l in range(L):
            lo, hi, pre = (int(v) for v in p.steps[j, l])
            if hi <= lo:
                continue
            if l == 0:
                a = self.x[:, :pre - p.c].to(dt)
                if p.c:
                    a = torch.cat((self.context, a), 1)
            else:
                a = self.acts[l - 1][:, :pre]
            self.acts[l][:, lo:hi] = torch.relu(F.linear(a, p.W[l][lo:hi, :pre], p.b[l][lo:hi]))
        pre = int(p.steps[j, L, 2])
        self.h.view(B, p.E, p.d)[:, :, j] = F.linear(self.acts[L - 1][:, :pre], p.W[L][j][:, :pre], p.b[L][j])
        return self.h


class MADE(nn.Module):
    def __init__(self, nin, hidden_sizes, nout, num_masks=1, natural_ordering=False, random=False, device="cpu"):
        super().__init__()
        assert nout % nin == 0, "nout must be integer multiple of nin"
        self.random, self.nin, self.nout, self.device = random, nin, nout, device
        self.pi = torch.tensor(math.pi).to(device)
        self.hidden_sizes = hidden_sizes
        sizes = [nin] + list(hidden_sizes) + [nout]
        layers = []
        for i in range(len(sizes) - 1):
            layers.append(MaskedLinear(sizes[i], sizes[i + 1]))
            if i < len(sizes) - 2:
                layers.append(nn.ReLU())
        self.net = nn.Sequential(*layers).to(device)
        self.natural_ordering, self.num_masks, self.seed = natural_ordering, num_masks, 0
        self.m = {}
        self._prog_static = None    # (key, device-resident index tensors + host step table) of progressive_plan
        self.update_masks()

    def _degrees(self):
        """Degree vectors m[-1] (inputs) and m[l] (hidden layer l)."""
        L = len(self.hidden_sizes)
        rng = np.random.RandomState(self.seed)
        self.seed = (self.seed + 1) % self.num_masks
        deg = {}
        if self.random:
            deg[-1] = np.arange(self.nin) if self.natural_ordering else rng.permutation(self.nin)
            for l in range(L):
                deg[l] = rng.randint(deg[l - 1].min(), self.nin - 1, size=self.hidden_sizes[l])
        else:
            deg[-1] = np.arange(self.nin)
            for l in range(L):
                deg[l] = (self.nin - 1) - (np.arange(self.hidden_sizes[l]) % self.nin)
        return deg

    def update_masks(self):
        if self.m and self.num_masks == 1:
            return
        L = len(self.hidden_sizes)
        self.m = self._degrees()
        masks = [self.m[l - 1][:, None] <= self.m[l][None, :] for l in range(L)]     # hidden: non-strict
        masks.append(self.m[L - 1][:, None] < self.m[-1][None, :])                   # output: strict
        if self.nout > self.nin:
            masks[-1] = np.tile(masks[-1], (1, self.nout // self.nin))
        for layer, mask in zip(self._masked_layers(), masks):
            layer.set_mask(mask)
        self.i_map = np.argsort(self.m[-1])

    def _masked_layers(self):
        return [l for l in self.net if isinstance(l, MaskedLinear)]

    # ---- progressive conditioner of the sequential sampling walk -----------------------------------------------------------------
    def _progressive_static(self, device):
        """The part of the plan that depends on the degrees only: orders, output rows, the step table.  None when ineligible."""
        layers = self._masked_layers()
        key = (str(device), tuple(l._epoch for l in layers))
        if self._prog_static is not None and self._prog_static[0] == key:
            return self._prog_static[1]
        nin, L = self.nin, len(self.hidden_sizes)
        c = getattr(self, "cond_in", 0)
        d, E = nin - c, self.nout // nin
        static = None
        if self.num_masks == 1 and L >= 1 and d >= 1 and np.array_equal(np.asarray(self.m[-1]), np.arange(nin)):
            if device.type == "cuda" and torch.cuda.is_current_stream_capturing():
                # (pageable host -> device copies cannot be recorded: graphs.GraphedSampler builds the plan before it captures)
                raise RuntimeError("MADE.progressive_plan: the plan tables must exist before a stream capture starts "
                                   "(umnn_amd.GraphedSampler primes them; call flow.invert(..., conditioner='progressive') once eagerly)")
            orders = [np.argsort(np.asarray(self.m[l]), kind="stable") for l in range(L)]
            sdeg = [np.asarray(self.m[l])[orders[l]] for l in range(L)]
            steps = np.zeros((d, L + 1, 3), dtype=np.int32)
            prev_hi = [0] * L
            for j in range(d):
                T = c + j - 1                       # units of degree <= T are final once x_0..x_{j-1} are
                for l in range(L):
                    hi = int(np.searchsorted(sdeg[l], T, side="right"))
                    steps[j, l] = (prev_hi[l], hi, c + j if l == 0 else steps[j, l - 1, 1])
                    prev_hi[l] = hi
                steps[j, L] = (0, E, steps[j, L - 1, 1])
            widths = [int(h) for h in self.hidden_sizes]
            ldk = [-(-k // 4) * 4 for k in [nin] + widths]
            out_rows = (np.arange(d)[:, None] + c + nin * np.arange(E)[None, :]).reshape(-1)       # [d][E] -> row e*nin + c + j
            static = dict(c=c, d=d, E=E, widths=widths, ldk=ldk, steps=steps,
                          max_new=int((steps[:, :L, 1] - steps[:, :L, 0]).max()),
                          orders=[torch.from_numpy(o).to(device) for o in orders], out_rows=torch.from_numpy(out_rows).to(device))
        self._prog_static = (key, static)
        return static

    def progressive_plan(self, device):
        """The plan of the progressive conditioner (``ProgressivePlan``), or None when this conditioner is not eligible: it needs the
        natural input order (m[-1] == arange(nin): the order ``UMNNMAF.invert`` walks), ``num_masks == 1`` and fp32 (or fp64) weights.
        By MADE's construction (``update_masks``) a hidden unit of degree m reads inputs of degree <= m and an output of dimension i
        hidden units of degree < i, so with c = cond_in (0 for MADE) step j of the walk computes every not-yet-computed unit of degree
        <= c + j - 1 (step 0 of a conditional block: all units of degree < c at once); a hidden layer's prefix is the count of previous
        -layer units of degree <= c + j - 1, the output's the count of last-hidden units of degree < c + j, layer 0's the c + j input
        columns; units of degree >= nin - 1 are never computed.  The permuted weights stay MASKED: their exact zeros make a prefix longer
        than one unit's own mask still exact.  Cached like the packed weights (``MaskedLinear._cached``, in the first layer's slots):
        keyed on weight / mask / bias versions and pointers, dropped by ``invalidate_caches`` and ``set_mask``."""
        layers = self._masked_layers()
        w0 = layers[0].weight
        if w0.dtype not in (torch.float32, torch.float64) or w0.device != device or any(l.bias is None for l in layers):
            return None
        static = self._progressive_static(device)
        if static is None:
            return None
        L = len(self.hidden_sizes)

        def build():
            with torch.no_grad():
                W, b = [], []
                for l in range(L):
                    w = (layers[l].mask * layers[l].weight).index_select(0, static["orders"][l])
                    if l > 0:
                        w = w.index_select(1, static["orders"][l - 1])
                    W.append(F.pad(w, (0, static["ldk"][l] - w.shape[1])).contiguous())
                    b.append(layers[l].bias.index_select(0, static["orders"][l]).contiguous())
                w = (layers[L].mask * layers[L].weight).index_select(0, static["out_rows"]).index_select(1, static["orders"][L - 1])
                W.append(F.pad(w, (0, static["ldk"][L] - w.shape[1])).view(static["d"], static["E"], static["ldk"][L]).contiguous())
                b.append(layers[L].bias.index_select(0, static["out_rows"]).view(static["d"], static["E"]).contiguous())
            return ProgressivePlan(static, W, b)
        return layers[0]._cached("plan", (str(device), w0.dtype) + tuple((l._epoch,) + l._key()[:6] for l in layers), build)

    # ---- the conditioner call: gather the inputs, ask for the route, run it ------------------------------------------------------
    def _kept_rows(self, device):
        return None                 # MADE keeps every output row

    def _drop_context(self, out):
        return out                  # ... and every output column

    def _raw(self, x, context, n_out, out_dtype):
        layers = self._masked_layers()
        w = layers[0].weight
        grad, autocast, graph = torch.is_grad_enabled(), torch.is_autocast_enabled(), _graph_mode()
        cuda_fp32 = x.is_cuda and (x.dtype if autocast else w.dtype) == torch.float32       # (of the input after _to_weight_dtype)
        needs_grad = (grad and not graph and x.dim() == 2 and all(l.weight.dtype == torch.float32 and l.bias is not None and l.weight.is_cuda for l in layers)
                      and (x.requires_grad or (context is not None and context.requires_grad)
                           or any(l.weight.requires_grad or l.bias.requires_grad for l in layers)))
        route = conditioner_route(x.shape[0], [(l.in_features, l.out_features) for l in layers], n_out, cuda_fp32,
                                  context is not None and x.dtype == torch.float32 == w.dtype, grad, needs_grad, autocast, graph,
                                  not graph and _probe(cuda_fp32, x.device), _OPTIONS)
        if context is None:
            a, a2 = _to_weight_dtype(x, layers[0]), None
        elif route.no_cat:                      # the kernel reads both blocks
            a, a2 = context, x
        else:
            a, a2 = _to_weight_dtype(torch.cat((context, x), 1), layers[0]), None
        # (graph mode computes every row and drops the context columns, as the reference does: no index tensor enters the graph)
        out = _run_route(route, a, a2, layers, None if graph else self._kept_rows(x.device), out_dtype)
        if route.name in _FAST_ROUTES:
            return out
        return _cast(self._drop_context(out) if graph else out, out_dtype)

    def raw(self, x, out_dtype=None):
        """The masked MLP itself (what the flow's EmbeddingNetwork needs, whatever nout is)."""
        return self._raw(x, None, self.nout, out_dtype)

    def graph_weights(self):
        """[mask * weight] of every masked linear, formed by ordinary torch ops: what a recorded caller that runs the conditioner
        many times on unchanged weights (the sampling loops of ``UMNNMAF.invert``) forms once and hands to ``raw_graph``."""
        return [l.mask * l.weight for l in self._masked_layers()]

    def _graph_chain(self, a, weights):
        layers = self._masked_layers()
        for i, (layer, w) in enumerate(zip(layers, weights)):
            a = F.linear(a, w, layer.bias)
            if i + 1 < len(layers):
                a = torch.relu(a)
        return a

    def raw_graph(self, x, weights, out_dtype=None):
        """``raw(x)`` in its graph-mode composition (fp32 F.linear + ReLU) on the masked weights of ``graph_weights()``."""
        return _cast(self._graph_chain(_to_weight_dtype(x, self.net[0]), weights), out_dtype)

    def raw_rows(self, x, rows):
        """Output COLUMNS ``rows`` (an int64 device tensor) of ``raw(x)`` only -> [B, len(rows)] fp32, or None when this
        conditioner / call is not one the restriction pays for (the caller then takes ``raw(x)``).  Sampling needs, per flow dimension
        j, the E embedding entries of that dimension out of E*d (UMNNMAF.invert, UMNNMAF.py:195-231, recomputes the whole MADE per
        dimension): for d = 784 the last masked linear is 23 520 rows of which 30 are read.  Inference path only (K-concatenated
        bf16 GEMMs): hidden layers as in ``raw``, the last layer as [B, 3K+2] x [3K+2, len(rows)] on the selected rows of its cached
        packed weight."""
        layers = self._masked_layers()
        x = _to_weight_dtype(x, layers[0])
        if len(layers) < 2 or layers[-1].out_features < 4096 or not _fast_path_ok(x):
            return None
        return _run_route(Route("split", False, False), x, None, layers, None, None, select=rows)

    def forward(self, x, context=None):
        if self.nout == 2:       # reference quirk (made.py:114-118): nout == 2 means "Gaussian MADE"
            out = self.net(x)
            mu, sigma = out[:, :self.nin], out[:, self.nin:]
            return (x - mu) * torch.exp(-sigma)
        return self.net(x)

    def compute_ll(self, x):
        out = self.net(x)
        mu, sigma = out[:, :self.nin], out[:, self.nin:]
        z = (x - mu) * torch.exp(-sigma)
        log_prob_gauss = -.5 * (torch.log(self.pi * 2) + z ** 2).sum(1)
        return -sigma.sum(1) + log_prob_gauss, z

    def invert(self, z):
        if self.nin != self.nout / 2:
            return None
        u = torch.zeros(z.shape)
        for d in range(self.nin):
            out = self.net(u)
            j = self.i_map[d]
            u[:, j] = z[:, j] * torch.exp(out[:, self.nin + j]) + out[:, j]
        return u


class ConditionnalMADE(MADE):
    """MADE over [context, x]; the context columns of every output chunk are dropped (made.py:165-168)."""

    def __init__(self, nin, cond_in, hidden_sizes, nout, num_masks=1, natural_ordering=False, random=False,
                 device="cpu"):
        super().__init__(nin + cond_in, hidden_sizes, nout, num_masks, natural_ordering, random, device)
        self.nin_non_cond, self.cond_in = nin, cond_in
        self._keep = None

    def _kept_rows(self, device):
        """Row indices of the last layer that survive the [:, :, cond_in:] slice, in output order."""
        if self._keep is None or self._keep.device != device:
            k = self.nout // self.nin
            idx = (torch.arange(k).view(-1, 1) * self.nin + torch.arange(self.cond_in, self.nin).view(1, -1))
            if device.type == "cuda" and torch.cuda.is_current_stream_capturing():
                # (a pageable host -> device copy cannot be recorded: graphs._prime_for_capture builds the indices before it captures)
                raise RuntimeError("ConditionnalMADE: the kept-row indices must exist before a stream capture starts "
                                   "(umnn_amd.GraphedLL / GraphedTrainStep prime them; call model(x) once eagerly otherwise)")
            self._keep = idx.reshape(-1).to(device)
        return self._keep

    def _drop_context(self, out):
        """The reference's ConditionnalMADE.forward (made.py:165-168): [B, k*nin] -> the non-context columns of every chunk."""
        return out.view(out.shape[0], out.shape[1] // self.nin, self.nin)[:, :, self.cond_in:].reshape(out.shape[0], -1)

    def raw(self, x, context, out_dtype=None):
        if context.dtype != x.dtype:
            context = context.to(x.dtype)
        return self._raw(x, context, self.nin_non_cond * (self.nout // self.nin), out_dtype)

    def raw_graph(self, x, context, weights, out_dtype=None):
        if context.dtype != x.dtype:
            context = context.to(x.dtype)
        out = self._graph_chain(_to_weight_dtype(torch.cat((context, x), 1), self.net[0]), weights)
        return _cast(self._drop_context(out), out_dtype)

    def forward(self, x, context):
        if self.nout == 2:
            return self._drop_context(super().forward(torch.cat((context, x), 1)))
        return self.raw(x, context)

    def computeLL(self, x, context):
        out = self.raw(x, context)
        n = self.nin_non_cond
        mu, sigma = out[:, :n], out[:, n:]
        z = (x - mu) * torch.exp(-sigma)
        log_prob_gauss = -.5 * (torch.log(self.pi * 2) + z ** 2).sum(1)
        return -sigma.sum(1) + log_prob_gauss, z
