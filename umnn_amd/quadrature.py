"""Clenshaw-Curtis tables (host logic).

Mirrors ``compute_cc_weights`` of the reference (models/UMNN/ParallelNeuralIntegral.py:14-34, duplicated at
NeuralIntegral.py:14-34 and UMNNMAF.py:55-69): same name, same return value
``(cc_weights[n+1,1], steps[n+1,1])`` as fp32 CPU tensors, same module-level cache.  The device copies the
HIP kernels read are cached per (n, device) so no host->device transfer happens on the hot path.
"""
import math

import numpy as np
import torch

_cc_weights_cache = {}
_device_cache = {}


def _tables_f64(nb_steps):
    """w = Lambda^T W in float64.  Lambda_jk = cos(jk*pi/n)*2/n with column 0 -> 1/n and column n halved;
    W_j = 2/(1-j^2) on even j (W_0 = 1), 0 on odd j.  Written with the node index leading so that the
    product is one matrix-vector contraction."""
    n = int(nb_steps)
    if n < 1:
        raise ValueError("nb_steps must be >= 1")
    idx = np.arange(n + 1)
    lam_t = np.cos(np.outer(idx, idx) * math.pi / n)       # [k, j] (symmetric before the edits)
    lam_t[0, :] = .5
    lam_t[-1, :] = .5 * lam_t[-1, :]
    lam_t = lam_t * 2 / n
    W = np.zeros(n + 1)
    even = idx[::2]
    W[even] = 2. / (1. - even.astype(np.float64) ** 2)
    W[0] = 1.
    return lam_t @ W, np.cos(idx * math.pi / n)


def compute_cc_weights(nb_steps):
    key = int(nb_steps)
    hit = _cc_weights_cache.get(key)
    if hit is None:
        w, s = _tables_f64(key)
        hit = (torch.from_numpy(w.reshape(-1, 1)).float(), torch.from_numpy(s.reshape(-1, 1)).float())
        _cc_weights_cache[key] = hit
    return hit


def device_tables(nb_steps, device):
    """Flat fp32 (w, s) on ``device``; uploaded once per (n, device)."""
    device = torch.device(device)
    key = (int(nb_steps), device.type, device.index)
    hit = _device_cache.get(key)
    if hit is None:
        w, s = compute_cc_weights(nb_steps)
        hit = (w.reshape(-1).contiguous().to(device), s.reshape(-1).contiguous().to(device))
        _device_cache[key] = hit
    return hit


_cumulative_cache = {}
_cumulative_device_cache = {}


def cc_cumulative_matrix(nb_steps):
    """Q, float64 [n+1, n+1]: the integral of the quadrature's own interpolant up to every node,

        int_{x0}^{t_i} f  =  (x - x0)/2 * sum_j Q[i, j] f(t_j),      t_j = x0 + (x - x0)(s_j + 1)/2,  s_j = cos(j pi / n).

    Built from the weight construction of ``_tables_f64``, not from a textbook DCT: Q = Wc @ lam_t.T with the same ``lam_t`` and
    Wc[i, j] = int_{-1}^{s_i} T_j(s) ds, column j = 0 halved (the ``W[0] = 1`` there).  Node 0 is x, so row 0 is the integral over
    the whole interval -- ``compute_cc_weights`` to float64 rounding, including the reference's unhalved last coefficient for even
    n -- and row n (the lower limit) is exactly zero.  Cached like the weights; callers must not modify it."""
    n = int(nb_steps)
    hit = _cumulative_cache.get(n)
    if hit is not None:
        return hit
    if n < 1:
        raise ValueError("nb_steps must be >= 1")
    idx = np.arange(n + 1)
    lam_t = np.cos(np.outer(idx, idx) * math.pi / n)       # exactly as in _tables_f64
    lam_t[0, :] = .5
    lam_t[-1, :] = .5 * lam_t[-1, :]
    lam_t = lam_t * 2 / n
    s = np.cos(idx * math.pi / n)

    def cheb(m):      # T_m at the nodes, [n+1, len(m)]: cos(m i pi / n) with the angle reduced, so that node n gives exactly +-1
        return np.cos(np.mod(np.outer(idx, m), 2 * n) * (math.pi / n))

    Wc = np.zeros((n + 1, n + 1))
    Wc[:, 0] = (s + 1.) / 2                                 # int T_0 = s + 1, halved
    Wc[:, 1] = (s * s - 1.) / 2
    if n >= 2:
        j = idx[2:].astype(np.float64)
        G = .5 * (cheb(idx[2:] + 1) / (j + 1) - cheb(idx[2:] - 1) / (j - 1))    # antiderivative of T_j, j >= 2
        Wc[:, 2:] = G - G[-1:, :]
    Q = Wc @ lam_t.T
    Q[-1, :] = 0.
    Q.setflags(write=False)
    _cumulative_cache[n] = Q
    return Q


def device_cumulative_matrix(nb_steps, device, ascending=False, dtype=torch.float32):
    """[n+1, n+1] copy of ``cc_cumulative_matrix`` on ``device`` (fp32: what the kernel reads), uploaded once per (n, device,
    dtype).  ``ascending``: the columns reversed, for values stored from the lower limit up (what a curve returns) rather than in
    node order (node 0 = x)."""
    device = torch.device(device)
    key = (int(nb_steps), device.type, device.index, bool(ascending), dtype)
    hit = _cumulative_device_cache.get(key)
    if hit is None:
        Q = cc_cumulative_matrix(nb_steps)
        Q = np.array(Q[:, ::-1] if ascending else Q)       # (a writable, contiguous copy)
        hit = _cumulative_device_cache[key] = torch.from_numpy(Q).to(dtype).contiguous().to(device)
    return hit


_adjoint_device_cache = {}


def device_cumulative_adjoint(nb_steps, device, ascending=False, dtype=torch.float32):
    """[n+1, n+1] table of the ADJOINT of the cumulative quadrature on ``device``, uploaded once per (n, device, ascending, dtype):
    Qt[j, i] = Q[n - i, j] with Q = ``device_cumulative_matrix(nb_steps, device, ascending)``'s entries -- that table transposed,
    its row index counted from the lower limit, as the cumulative quadrature's ascending output is.  For a cotangent g [B, n+1, K] of
    that output, sum_i Qt[j, i] g[:, i] is the cotangent of the values at node j up to the factor (x - x0)/2: in node order (node 0
    = x), or -- ``ascending`` -- from the lower limit up, like the values ``cumulate`` takes."""
    device = torch.device(device)
    key = (int(nb_steps), device.type, device.index, bool(ascending), dtype)
    hit = _adjoint_device_cache.get(key)
    if hit is None:
        Q = cc_cumulative_matrix(nb_steps)
        Q = Q[::-1, ::-1] if ascending else Q[::-1, :]
        hit = _adjoint_device_cache[key] = torch.from_numpy(np.array(Q.T)).to(dtype).contiguous().to(device)
    return hit
