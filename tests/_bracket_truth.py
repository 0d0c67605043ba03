"""Float64 restatement of the bracket search of umnn_flow_invert_dim, written from the description in include/umnn_cc.h and the
kernel (cc_fwd_bf16_kernel.h, INV = 1) on top of the numpy oracle's quadrature.  It shares no code with ``UMNNMAF._invert`` or the
kernels it is compared with.

The search, per row: the bracket starts as [-50, 50]; a round places ten candidates at left + (p / 9) span, p = 0..9, takes their
images G = exp(scaling_j) (h[b, 0 d + j] + int_0^cand f(t; h[b, :, j]) dt), picks the candidate whose image is nearest the target
(ties: the lower p) and keeps [best, next] when that image lies below the target, [prev, best] otherwise.  After k rounds the bracket
is one candidate step of round k wide: 100 / 9^k.

``grid`` is the number format of the bracket arithmetic alone.  np.float64: the search as mathematics.  np.float32: the candidates
the kernel forms, fl(fl(fl(p / 9) span) + left) with span = fl(right - left) -- the images are float64 either way, so for a row whose
decisions are not marginal this run makes the kernel's decisions and ends on the kernel's candidate to one fp32 ulp of 50 (the
compiler may contract the product and the sum of that formula into one fma: measured on gfx950, fma(fl(4 / 9), 100, -50) = -5.5555553
where the two roundings give -5.5555534)."""
import types

import numpy as np

from oracle import cc_oracle as O

K = 10                                   # candidates per round
ULP_50 = 2.0 ** -18                      # one fp32 ulp of a value in [32, 64): the returned candidates lie in [-50, 50]


def bracket64(net, h_j, z_j, log_scale_j, n, iters, grid=np.float64):
    """``iters`` rounds for the rows of h_j [B, E] (the embedding of one dimension, row 0 the offset) and targets z_j [B].
    -> (best candidate of the last round [B] in ``grid``, decision margin [B]): the margin of a row is the minimum over its rounds of
    the gap between the smallest and the second smallest distance |G - z| and of |G_best - z|, the two quantities whose sign the
    round's two decisions (which candidate, which side) turn on."""
    h_j = np.asarray(h_j, np.float64)
    z = np.asarray(z_j, np.float64).reshape(-1)
    B = z.size
    frac = (np.arange(K) / 9.0).astype(grid)
    left, right = np.full(B, -50., grid), np.full(B, 50., grid)
    best = np.zeros(B, grid)
    margin = np.full(B, np.inf)
    scale, off = np.exp(np.float64(log_scale_j)), h_j[:, 0]
    h_rep = np.repeat(h_j, K, axis=0)                                     # row b K + p
    rows = np.arange(B)
    for _ in range(int(iters)):
        span = right - left
        cand = (frac[None, :] * span[:, None]).astype(grid) + left[:, None]
        assert cand.dtype == grid
        c64 = cand.astype(np.float64).reshape(-1, 1)
        F = O.integrate_parallel(net, np.zeros_like(c64), c64, h_rep, n).reshape(B, K)
        G = scale * (off[:, None] + F)
        dist = np.abs(G - z[:, None])
        m = np.argmin(dist, axis=1)                                       # (first occurrence: the lower p)
        d_best = dist[rows, m]
        d_second = np.partition(dist, 1, axis=1)[:, 1]
        margin = np.minimum(margin, np.minimum(d_second - d_best, d_best))
        below = G[rows, m] < z
        lo, hi = cand[rows, np.maximum(m - 1, 0)], cand[rows, np.minimum(m + 1, K - 1)]
        best = cand[rows, m]
        left, right = np.where(below, best, lo), np.where(below, hi, best)
    return best, margin


def flow_bracket64(blocks, z, n, iters):
    """UMNNMAFFlow.invert(z, iter=iters) with ``bracket64`` as the search of every dimension and the oracle's MADE as conditioner:
    the blocks in reverse order, the dimensions flipped between blocks, within a block dimension by dimension."""
    z = np.asarray(z, np.float64)[:, ::-1]
    for blk in reversed(blocks):
        z = z[:, ::-1]
        B, d = z.shape
        x = np.zeros_like(z)
        for j in range(d):
            h = blk.embed(x)
            x[:, j] = bracket64(blk.net, h.reshape(B, -1, d)[:, :, j], z[:, j], blk.scaling[j], n, iters)[0]
        z = x
    return z


# ---- the inputs of tests/test_gpu_invert_coverage.py (built on the CPU, so that the CPU tests can run the same cases) -------------
D = 3
_CASES = {}
# Seeds of the B = 37 cases: for each net the first seed in 0, 1, 2, ... at which the float64 search leaves out at most 2 of the 37
# rows (check (b): the cap is 10 %, i.e. 3 rows; the expected share is about 3 %) for n in (20, 2), j in (0, 2) and iters in (4, 1).
# Found on the CPU with the float64 restatement alone; nets that are not listed use seed 0.
SEEDS = {((60, 60, 60), 4): 1, ((70, 90), 4): 1, ((80, 80, 80, 80), 4): 1}


def seed_of(hid, E):
    return SEEDS.get((tuple(hid), E), 0)


def oracle_net(net, hidden_act=O.LEAKY):
    import torch
    lins = [m for m in net.net if isinstance(m, torch.nn.Linear)]
    return O.Net([l.weight.detach().cpu().double().numpy() for l in lins], [l.bias.detach().cpu().double().numpy() for l in lins],
                 hidden_act, O.ELU1)


def case(hid, E, B, n, seed=0):
    """One default-initialised IntegrandNetwork(D, 1 + E, hid, 1) with x ~ 1.5 N(0, 1) [B, D], h ~ N(0, 1) [B, E D], scaling ~ 0.3 N(0, 1)
    [D] and the float64 targets z64 = exp(scaling) (h[:, 0 D + j] + int_0^x f), computed once per key and never modified.  The float64
    searches of a case are cached on it by ``truth``."""
    import torch
    import umnn_amd
    key = (tuple(hid), E, B, n, seed)
    if key not in _CASES:
        torch.manual_seed(1000 * seed + 31 * len(hid) + hid[0] + E)
        net = umnn_amd.IntegrandNetwork(D, 1 + E, list(hid), 1)
        onet = oracle_net(net)
        g = torch.Generator().manual_seed(7919 * seed + 131 * B + n)
        x = torch.randn(B, D, generator=g, dtype=torch.float64) * 1.5
        h = torch.randn(B, E * D, generator=g)
        scaling = 0.3 * torch.randn(D, generator=g)
        xn, hn, sn = x.numpy(), h.double().numpy(), scaling.double().numpy()
        z64 = np.exp(sn)[None, :] * (hn[:, :D] + O.integrate_parallel(onet, np.zeros_like(xn), xn, hn, n))
        _CASES[key] = types.SimpleNamespace(net=net, onet=onet, hid=list(hid), E=E, B=B, n=n, xn=xn, hn=hn, sn=sn, h=h, scaling=scaling,
                                            z64=z64, z=torch.from_numpy(z64).float(), f64=O.integrand(onet, xn, hn), searches={})
    return _CASES[key]


def truth(c, j, iters):
    """``bracket64`` on the kernel's fp32 grid for column j of case ``c``, against the fp32 targets the kernel reads -> (best, margin)."""
    if (j, iters) not in c.searches:
        h_j = c.hn.reshape(c.B, c.E, D)[:, :, j]
        c.searches[(j, iters)] = bracket64(c.onet, h_j, c.z[:, j].double().numpy(), c.sn[j], c.n, iters, grid=np.float32)
    return c.searches[(j, iters)]


def truth_bound(c, j, grid_step, tol, rows=slice(None)):
    """[rows] bound of |x_hat - x|: the grid spacing of the last round plus what a forward error of ``tol`` max(1, |z|) can move a
    decision by, tol max(1, |z|) / (exp(scaling_j) min f) with min f the float64 integrand's minimum over the rows."""
    z = np.abs(c.z64[rows, j])
    return grid_step + tol * np.maximum(1., z) / (np.exp(c.sn[j]) * float(c.f64[rows, j].min()))


# ---- the tables of tests/test_gpu_invert_coverage.py and tests/test_bracket_cpu.py ---------------------------------------------------
TOL = 1e-4                               # the forward parity tolerance of the project
JS = (0, D - 1)
STEP6 = 100. / 9 ** 6
# t_out = (H + 16) // 16 tiles and ks_in = (H + 4) // 4 live registers per layer of width H (umnn_prepare_mlp); a uniform net of five to
# eight tiles runs on eight waves once 2 (image bytes + 1024) exceeds 160 KiB; a first layer of five to eight tiles over layers of at
# most four takes the wide-first family.  The plan is that of cc_solve.hip (tests/test_gpu_solve_coverage.py has the same nets).
# (net, E, name after the build's prefix)
TWO_PIECE = [
    ([50] * 4, 30, "<T=4,EXACT=1,LIVE=13>"),
    ([60] * 3, 4, "<T=4,EXACT=1,LIVE=0>"),
    ([40, 33], 4, "<T=4,EXACT=1,LIVE=0>"),                    # three tiles, zero-padded to four
    ([100, 100], 2, "<T=7,EXACT=1,LIVE=26>"),
    ([96, 96], 3, "<T=7,EXACT=1,LIVE=0>"),
    ([64, 64], 5, "<T=5,EXACT=1,LIVE=0>"),
    ([80, 80, 80], 6, "<T=6,EXACT=1,LIVE=0>"),
    ([112, 112], 7, "<T=8,EXACT=1,LIVE=0>"),
    ([100] * 3, 2, "<T=7,EXACT=1,LIVE=26,WAVES=8>"),
    ([96] * 3, 9, "<T=7,EXACT=1,LIVE=0,WAVES=8>"),
    ([64] * 5, 3, "<T=5,EXACT=1,LIVE=0,WAVES=8>"),
    ([80] * 4, 4, "<T=6,EXACT=1,LIVE=0,WAVES=8>"),
    ([127] * 3, 5, "<T=8,EXACT=1,LIVE=0,WAVES=8>"),
    ([20, 20], 4, "<T=2,EXACT=0,LIVE=0>"),
    ([70, 90], 4, "<T=8,EXACT=0,LIVE=0>"),
    ([64, 50, 50, 50], 8, "<T1=5,TREST=4,LIVE=13>"),
    ([80, 50, 50, 50], 8, "<T1=6,TREST=4,LIVE=13>"),
    ([100, 50, 50, 50], 8, "<T1=7,TREST=4,LIVE=13>"),
    ([127, 50, 50, 50], 8, "<T1=8,TREST=4,LIVE=13>"),
    ([79, 60, 60], 6, "<T1=5,TREST=4,LIVE=0>"),
    ([95, 63, 33], 6, "<T1=6,TREST=4,LIVE=0>"),
    ([111, 60, 60], 6, "<T1=7,TREST=4,LIVE=0>"),
    ([112, 20, 50], 6, "<T1=8,TREST=4,LIVE=0>"),
]
THREE_PIECE = [
    ([50] * 4, 30, "<T=4,PARTS=3,EXACT=1,LIVE=13>"),
    ([60] * 3, 4, "<T=4,PARTS=3,EXACT=1,LIVE=0>"),
    ([20, 20], 4, "<T=2,PARTS=3,EXACT=0,LIVE=0>"),
]
# Rows of kInvVariants no net can reach, with the reason from the plan of cc_invert.hip:
UNREACHABLE = [
    ("cc_invert_f16<T=4,EXACT=0,LIVE=0>", "a net of three or four tiles per layer is exact or is zero-padded to <T=4,EXACT=1,LIVE=0>"),
    ("cc_invert_bf16<T=4,EXACT=0,LIVE=0>", "a net of three or four tiles per layer is exact or is zero-padded to <T=4,EXACT=1,LIVE=0>"),
    ("cc_invert_bf16<T=4,PARTS=3,EXACT=0,LIVE=0>", "the zero-padding applies to three pieces as well: <T=4,PARTS=3,EXACT=1,LIVE=0>"),
]
# (precision, kernel name, net, E)
VARIANTS = ([("f16x3", "cc_invert_f16" + name, hid, E) for hid, E, name in TWO_PIECE]
            + [("bf16x3", "cc_invert_bf16" + name, hid, E) for hid, E, name in TWO_PIECE]
            + [("fp32", "cc_invert_bf16" + name, hid, E) for hid, E, name in THREE_PIECE]
            + [("bf16x6", "cc_invert_bf16<T=4,PARTS=3,EXACT=1,LIVE=13>", [50] * 4, 30),
               # above four tiles per layer the three-piece form does not exist: the two-fp16-piece search
               ("fp32", "cc_invert_f16<T=7,EXACT=1,LIVE=26>", [100, 100], 2),
               ("bf16x6", "cc_invert_f16<T1=7,TREST=4,LIVE=13>", [100, 50, 50, 50], 8)])
# the kernel of the flow-shaped net [50]*4, E = 30 under every precision
FLOW_NAME = {"f16x3": "cc_invert_f16<T=4,EXACT=1,LIVE=13>", "bf16x3": "cc_invert_bf16<T=4,EXACT=1,LIVE=13>",
             "bf16x6": "cc_invert_bf16<T=4,PARTS=3,EXACT=1,LIVE=13>", "fp32": "cc_invert_bf16<T=4,PARTS=3,EXACT=1,LIVE=13>"}
# one net per kernel family (and the three builds of the first)
FAMILIES = [("f16x3", FLOW_NAME["f16x3"], [50] * 4, 30),
            ("f16x3", "cc_invert_f16<T=7,EXACT=1,LIVE=26,WAVES=8>", [100] * 3, 2),
            ("f16x3", "cc_invert_f16<T1=7,TREST=4,LIVE=13>", [100, 50, 50, 50], 8),
            ("f16x3", "cc_invert_f16<T=2,EXACT=0,LIVE=0>", [20, 20], 4),
            ("bf16x3", FLOW_NAME["bf16x3"], [50] * 4, 30),
            ("fp32", FLOW_NAME["fp32"], [50] * 4, 30)]
FAMILY_IDS = [f"{p}-{'x'.join(map(str, hid))}" for p, _, hid, _ in FAMILIES]
# (net, E, waves per workgroup, kernel name)
SPLIT_EDGES = [([50] * 4, 30, 4, "cc_invert_f16<T=4,EXACT=1,LIVE=13>"), ([100, 50, 50, 50], 8, 4, "cc_invert_f16<T1=7,TREST=4,LIVE=13>"),
               ([100, 100], 2, 4, "cc_invert_f16<T=7,EXACT=1,LIVE=26>"), ([100] * 3, 2, 8, "cc_invert_f16<T=7,EXACT=1,LIVE=26,WAVES=8>")]
# the nets of the unsplit-plan tests: (net, E, waves per workgroup, kernel name by precision)
BIG = {"flow_50x4": ([50] * 4, 30, 4, FLOW_NAME),
       "waves8_100x3": ([100] * 3, 2, 8, {"f16x3": "cc_invert_f16<T=7,EXACT=1,LIVE=26,WAVES=8>"}),
       "wide_first": ([100, 50, 50, 50], 8, 4, {"f16x3": "cc_invert_f16<T1=7,TREST=4,LIVE=13>"})}
