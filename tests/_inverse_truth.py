"""Float64 truth for the inverse direction: a safeguarded solve written here, on top of the numpy oracle's forward maps
(``oracle.cc_oracle.integrate_parallel`` / ``monotonic_forward`` / ``block_forward``).  It shares no code with
``umnn_amd.integral.newton_solve`` or the kernels it is compared with."""
import numpy as np

from oracle import cc_oracle as O
from tests import _util as U


def net64(net):
    return O.Net([W.astype(np.float64) for W in net.Ws], [b.astype(np.float64) for b in net.bs], net.hidden_act, net.out_act)


def solve64(G, y, lo=-50., hi=50., max_iter=200):
    """x in [lo, hi] with G(x) = y for an increasing G: ``G(x) -> (value, derivative)``, elementwise on float64 arrays.  Newton from
    the bracket's midpoint, bisection whenever the step leaves the bracket; a y outside [G(lo), G(hi)] returns that endpoint."""
    y = np.asarray(y, np.float64)
    a, b = np.full_like(y, lo), np.full_like(y, hi)
    below, above = y <= G(a)[0], y >= G(b)[0]
    x = 0.5 * (a + b)
    for _ in range(max_iter):
        g, dg = G(x)
        r = g - y
        b = np.where(r > 0, x, b)
        a = np.where(r <= 0, x, a)
        with np.errstate(divide="ignore", invalid="ignore"):
            xn = x - r / dg
        xn = np.where((xn > a) & (xn < b), xn, 0.5 * (a + b))
        step = np.max(np.abs(xn - x) / np.maximum(np.abs(x), 1.0)) if x.size else 0.0
        x = xn
        if step <= 4e-16:
            break
    return np.where(below, lo, np.where(above, hi, x))


def newton64(G, target, lo=-50., hi=50., tol=1e-6, max_iter=64):
    """The iteration ``include/umnn_cc.h`` describes for umnn_cc_solve, restated in float64 row by row (no code shared with
    ``umnn_amd.integral.newton_solve``): start at 0 clamped into [lo, hi]; every evaluation G(x) -> (value, derivative) gives the
    residual r, whose sign moves one end of the bracket to x; the next point is x - r / G'(x), replaced -- when it is not strictly
    inside the bracket -- by the endpoint it overshot (each endpoint once, and only while no evaluation has replaced it) or by the
    bracket's midpoint.  A row stops when |r| <= tol max(1, |target|), when x sits on the endpoint the target lies beyond (clamped),
    when the midpoint no longer separates the ends or when the next point equals x; a row still running after ``max_iter``
    evaluations keeps its last evaluated x (capped).  -> (x, evaluations, clamped, capped), each shaped like ``target``."""
    t = np.asarray(target, np.float64)
    shape = t.shape
    t = t.reshape(-1)
    N = t.size
    x = np.full(N, min(max(0., lo), hi))
    a, b = np.full(N, float(lo)), np.full(N, float(hi))
    a_fresh, b_fresh = np.ones(N, bool), np.ones(N, bool)
    running = np.ones(N, bool)
    evals = np.zeros(N, np.int64)
    clamped = np.zeros(N, bool)
    for it in range(int(max_iter)):
        if not running.any():
            break
        g, dg = G(x.reshape(shape))
        g, dg = np.asarray(g, np.float64).reshape(-1), np.asarray(dg, np.float64).reshape(-1)
        for i in np.flatnonzero(running):
            evals[i] += 1
            r = g[i] - t[i]
            if abs(r) <= tol * max(1., abs(t[i])) and np.isfinite(r):      # (no x meets an infinite target)
                running[i] = False
                continue
            if r > 0:
                if x[i] <= lo:
                    clamped[i], running[i] = True, False
                b[i], b_fresh[i] = x[i], False
            else:
                if x[i] >= hi:
                    clamped[i], running[i] = True, False
                a[i], a_fresh[i] = x[i], False
            if not running[i]:
                continue
            nxt = x[i] - r / dg[i]
            if not (a[i] < nxt < b[i]):
                if nxt >= b[i] and b_fresh[i]:
                    nxt, b_fresh[i] = b[i], False
                elif nxt <= a[i] and a_fresh[i]:
                    nxt, a_fresh[i] = a[i], False
                else:
                    nxt = 0.5 * (a[i] + b[i])
                    if not (a[i] < nxt < b[i]):
                        running[i] = False
                        continue
            if nxt == x[i]:
                running[i] = False
            elif it + 1 < max_iter:
                x[i] = nxt
    return x.reshape(shape), evals.reshape(shape), clamped.reshape(shape), running.reshape(shape)


def integral_map(net, h, n, scale=1., off=0.):
    """G(x) -> (scale (off + int_0^x f), scale f(x)) in float64 for the rows of ``h`` (d = 1): the map umnn_cc_solve inverts."""
    h = np.asarray(h, np.float64)

    def G(x):
        x = np.asarray(x, np.float64)
        return scale * (off + O.integrate_parallel(net, np.zeros_like(x), x, h, n)), scale * O.integrand(net, x, h)
    return G


# ---- MonotonicNN -------------------------------------------------------------------------------------------------
def monotonic_parts(G):
    """float64 (integrand Net, conditioner Ws, bs) of a g5_monotonic fixture."""
    sd = U.state_dict_of(G)
    iW, ib, _ = U._seq(sd, "integrand.net.", np.float64)
    cW, cb, _ = U._seq(sd, "net.", np.float64)
    return O.Net(iW, ib, O.RELU, O.ELU1), cW, cb


def monotonic_map(net, cW, cb, h, n):
    """G(x) -> (y, dy/dx) of MonotonicNN.forward in float64 for the rows of ``h``."""
    h = np.asarray(h, np.float64)
    a = h
    for l, (W, b) in enumerate(zip(cW, cb)):
        a = a @ W.T + b
        if l < len(cW) - 1:
            a = np.maximum(a, 0.)
    scale = np.exp(a[:, [1]])

    def G(x):
        return O.monotonic_forward(net, cW, cb, x, h, n), scale * O.integrand(net, x, h)
    return G


# ---- flow --------------------------------------------------------------------------------------------------------
def blocks_from_state_dict(sd, nb_flow):
    """float64 oracle blocks of an unconditional UMNNMAFFlow from its state_dict (numpy arrays or tensors)."""
    sd = {k: np.asarray(v.detach().cpu() if hasattr(v, "detach") else v) for k, v in sd.items()}
    blocks = []
    for i in range(nb_flow):
        mW, mb, mm = U._seq(sd, f"Flow{i}.net.made.net.", np.float64)
        iW, ib, _ = U._seq(sd, f"Flow{i}.net.parallel_nets.net.", np.float64)
        blocks.append(O.Block(mW, mb, mm, O.Net(iW, ib, O.LEAKY, O.ELU1), sd[f"Flow{i}.scaling"].astype(np.float64)))
    return blocks


def blocks64(blocks):
    return [O.Block([W.astype(np.float64) for W in b.made_Ws], [v.astype(np.float64) for v in b.made_bs], b.made_masks, net64(b.net),
                    b.scaling.astype(np.float64), b.cond_in) for b in blocks]


def block_invert64(blk, z, n):
    """x with block_forward(blk, x) = z, dimension by dimension (the conditioner is autoregressive) -> (x, min exp(s) f(x))."""
    z = np.asarray(z, np.float64)
    B, d = z.shape
    x = np.zeros_like(z)
    for j in range(d):
        h = blk.embed(x)
        off = h.reshape(B, -1, d)[:, 0, j]

        def G(c, j=j, h=h, off=off):
            xx = x.copy()
            xx[:, j] = c
            F = O.integrate_parallel(blk.net, np.zeros_like(xx), xx, h, n)[:, j]
            return np.exp(blk.scaling[j]) * (F + off), np.exp(blk.scaling[j]) * O.integrand(blk.net, xx, h)[:, j]
        x[:, j] = solve64(G, z[:, j])
    h = blk.embed(x)
    return x, float(np.min(np.exp(blk.scaling)[None, :] * O.integrand(blk.net, x, h)))


def flow_invert64(blocks, z, n):
    """Inverse of ``O.flow_forward`` in float64 -> (x, [min exp(s) f of every block, in flow order])."""
    z = np.asarray(z, np.float64)[:, ::-1]
    mins = []
    for blk in reversed(blocks):
        z, m = block_invert64(blk, z[:, ::-1], n)
        mins.append(m)
    return z, mins[::-1]


def flow_min_sf(blocks, x, n):
    """min over rows and dimensions of exp(s) f(x; h) of every block along the forward pass of ``x`` (float64)."""
    x = np.asarray(x, np.float64)
    mins = []
    for blk in blocks:
        z, h = O.block_forward(blk, x, n)
        mins.append(float(np.min(np.exp(blk.scaling)[None, :] * O.integrand(blk.net, x, h))))
        x = z[:, ::-1]
    return mins
