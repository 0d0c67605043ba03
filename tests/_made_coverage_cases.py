"""Case tables, float64 truths and bounds of the conditioner and training-glue coverage tests: tests/test_made_coverage_cpu.py (names,
truths, input conditions, argument errors; no GPU) and tests/test_gpu_made_coverage.py (every case on the device).

Kernels.  csrc/made_fused.hip: made_fused_kernel<RT=1|4> (umnn_made_mlp_forward_ex, output modes 0 fp32, 1 bf16, 2 split3 operand) and
the nine made_linear_kernel<RT,TPC,PD,NW> (umnn_made_linear_forward); csrc/made_split.hip; csrc/made_train.hip (ReLU backward + bias
gradient: a vector branch for N % 4 == 0, a scalar branch otherwise, and the finish kernel); csrc/cc_flow_glue.hip (block cotangents,
ll forward, ll backward).

Names.  Written by hand from the launchers for a device of 256 CUs (fused_name / linear_plan restate the rules and the CPU test holds
the table against them):
  * made_fused: RT = 4 iff ceil(B / 64) >= cus // 2, i.e. from B = 8129 on 256 CUs (fused_threshold).
  * made_linear: T = ceil(N / 16) tiles, G groups (clipped to T), TG = ceil(T / G) tiles in the fullest workgroup: TG <= 4 ->
    TPC=1,NW=4; TG <= 8 -> TPC=1,NW=8; else TPC=2,NW=8.  PD (fragment ring depth) = 16 for TPC=1 at RT = 1, 2 and 8 otherwise.  At
    N = 1000 (T = 63): G = 16 -> TG 4, G = 8 -> TG 8, G = 3 -> TG 21 (two passes), G = 1 -> TG 63 (four passes), G = 500 -> clipped to
    63 groups of one tile.

Arithmetic under test (one masked linear):  y = hi(a) hi(W) + lo(a) hi(W) + hi(a) lo(W) + b with hi = bf16_rn(.), lo = bf16_rn(. - hi),
fp32 accumulation; a = relu(input) where the kernel applies ReLU before the split; lo(a) lo(W) is dropped.

Truths.  exact_layer: the layer in float64 on the float32 values.  emu_layer: the three products above in float64.  E32 = max(e32,
2^-22), e32 = the error of the same single layer in float32 torch on the CPU against exact_layer, over max|exact|.  A kernel's single
layer must be within M x E32 x max|emu| of emu (M = 8: the constant of the forward coverage for its fp32-level modes; an fp32
accumulation of the three products in another order than torch's stays a small multiple of e32).  Deep nets are tested by peeling
(layer l of the depth-l prefix against emu of layer l on the ReLU of the kernel's own depth-(l-1) output), because an emulated CHAIN
and the kernel's chain part by the dropped lo lo term as soon as a hidden value rounds differently.  The whole chain against the
float64 MLP keeps the project's 2e-5 x max|exact|; the inputs are chosen so that the emulated chain alone stays under 1e-5 (CPU test).

Inputs.  random_net: W = randn / sqrt(K) under a mask that keeps 60 % of the entries, b uniform in [-1, 1], x = 2 randn, fixed seeds.
exact_net: x integers in [-8, 8], b integers in [-2, 2], every weight row at most two non-zeros from {-1, 1}: every split is exact, the
low weight pieces are zero, every partial sum is an integer below 2^16 through eight layers (|y| <= 2 max|a| + 2: 8 -> 2558), so fp32
accumulation is exact in any order and the kernel must equal exact bit for bit.  exact_weight(N, K, r) puts the two non-zeros of row
16 t + rho at k = 32 ((t + r) mod S) + 2 rho and the next: over r = 0 .. S - 1 every (output tile, K-step, lane group, slot) of the
fragment layout carries a weight at least once (the `shifts` of a case)."""
import ctypes

import torch

from umnn_amd import _lib

M = 8.0
FLOOR = 2.0 ** -22
WHOLE_CHAIN = 2e-5          # the project's bound of the conditioner fast path against the float64 MLP
EMU_CHAIN = 1e-5            # what the emulated chain alone must stay under (input condition)
CUS_REF = 256
GUARD = 64                  # elements behind every output that must stay untouched

FUSED_NAMES = ["made_fused<RT=1>", "made_fused<RT=4>"]
LINEAR_VARIANTS = [(rt, tpc, (8 if rt == 4 or tpc == 2 else 16), nw) for rt in (1, 2, 4) for tpc, nw in ((1, 4), (1, 8), (2, 8))]


def linear_name(rt, tpc, pd, nw):
    return f"made_linear<RT={rt},TPC={tpc},PD={pd},NW={nw}>"


LINEAR_NAMES = [linear_name(*v) for v in LINEAR_VARIANTS]


# ---- launcher rules, restated ----------------------------------------------------------------------------------------------------------
def fused_name(B, cus):
    return FUSED_NAMES[1] if -(-B // 64) >= cus // 2 else FUSED_NAMES[0]


def fused_threshold(cus):
    """Smallest B that runs made_fused<RT=4>: its last workgroup holds one row."""
    return 64 * (cus // 2 - 1) + 1


def linear_plan(B, N, rt, fg, cus):
    """(name, RT, G, TG) of umnn_made_linear_forward(row_tiles=rt, feature_groups=fg)."""
    T = -(-N // 16)
    gmax = T // 4 if T >= 4 else 1
    RT, G = rt, fg
    if RT == 0:
        RT = 1
        for r in (4, 2, 1):
            if -(-B // (16 * r)) * gmax >= cus or r == 1:
                RT = r
                break
    if G == 0:
        rows = -(-B // (16 * RT))
        G = max(1, min(gmax, -(-cus // rows)))
    G = min(G, T)
    TG = -(-T // G)
    tpc, nw = ((1, 4) if TG <= 4 else (1, 8) if TG <= 8 else (2, 8))
    pd = 8 if RT == 4 or tpc == 2 else 16
    return linear_name(RT, tpc, pd, nw), RT, G, TG


# ---- arithmetic -------------------------------------------------------------------------------------------------------------------------
def split(a32):
    """(hi, lo) bf16 pieces of a float32 tensor, as float64."""
    hi = a32.bfloat16()
    lo = (a32 - hi.float()).bfloat16()
    return hi.double(), lo.double()


def exact_layer(a32, W32, b32, relu_in):
    a = torch.relu(a32) if relu_in else a32
    return a.double() @ W32.double().t() + b32.double()


def emu_layer(a32, W32, b32, relu_in, pieces=None):
    """The kernel's stated arithmetic in float64; ``pieces`` = (Wh, Wl) float64 replaces the plain split of W32."""
    a = torch.relu(a32) if relu_in else a32
    ah, al = split(a)
    Wh, Wl = split(W32) if pieces is None else pieces
    return ah @ Wh.t() + al @ Wh.t() + ah @ Wl.t() + b32.double()


def f32_layer(a32, W32, b32, relu_in):
    a = torch.relu(a32) if relu_in else a32
    return a @ W32.t() + b32


def e32_of(f32_value, exact):
    return float((f32_value.double() - exact).abs().max() / exact.abs().max().clamp_min(1e-300))


def layer_truth(a32, W32, b32, relu_in):
    """(emu, E32) of one layer on the CPU: what a kernel's output of that layer is held against."""
    a32, W32, b32 = a32.cpu(), W32.cpu(), b32.cpu()
    ex = exact_layer(a32, W32, b32, relu_in)
    return emu_layer(a32, W32, b32, relu_in), max(e32_of(f32_layer(a32, W32, b32, relu_in), ex), FLOOR)


def layer_ratio(got, emu, E32):
    """err / E32 of a kernel output against emu (must be <= M)."""
    scale = float(emu.abs().max().clamp_min(1e-300))
    return float((got.double().cpu() - emu).abs().max()) / scale / E32


def exact_chain(Ws, bs, x):
    a = x.double()
    for l, (W, b) in enumerate(zip(Ws, bs)):
        a = a @ W.double().t() + b.double()
        if l + 1 < len(Ws):
            a = torch.relu(a)
    return a


def emu_chain(Ws, bs, x):
    """Every layer by emu_layer, the hidden values rounded to float32 in between (as the kernel holds them)."""
    a = x
    for l, (W, b) in enumerate(zip(Ws, bs)):
        a = emu_layer(a, W, b, l > 0)
        if l + 1 < len(Ws):
            a = a.float()
    return a


def unpack_fragments(frag, N, K):
    """(Wh, Wl) float64 [N, K] out of pack_fragments' [T, S, 2, 64, 8] -- the inverse of the layout the kernels read."""
    T, S = frag.shape[0], frag.shape[1]
    lane = torch.arange(64)
    g, rho = lane >> 4, lane & 15
    j = torch.arange(8)
    n = (16 * torch.arange(T).view(T, 1, 1, 1) + rho.view(1, 1, 64, 1)).expand(T, S, 64, 8)
    k = (32 * torch.arange(S).view(1, S, 1, 1) + (16 * (j >> 2) + (j & 3)).view(1, 1, 1, 8) + 4 * g.view(1, 1, 64, 1)).expand(T, S, 64, 8)
    out = []
    for piece in range(2):
        Wp = torch.zeros(16 * T, 32 * S, dtype=torch.float64)
        Wp[n.reshape(-1), k.reshape(-1)] = frag[:, :, piece].double().reshape(-1)
        assert Wp[N:].abs().max().item() == 0 if 16 * T > N else True
        assert Wp[:, K:].abs().max().item() == 0 if 32 * S > K else True
        out.append(Wp[:N, :K].contiguous())
    return out


def split3_torch(x, relu, ld):
    """umnn_made_split3's operand [hi | lo | hi | 1 | 1 | 0 ...] restated in torch (the form test_made_split3_edge_shapes uses)."""
    rows, cols = x.shape
    a = torch.relu(x) if relu else x
    hi = a.bfloat16()
    lo = (a - hi.float()).bfloat16()
    return torch.cat([hi, lo, hi, torch.ones(rows, 2, dtype=torch.bfloat16, device=x.device),
                      torch.zeros(rows, ld - 3 * cols - 2, dtype=torch.bfloat16, device=x.device)], 1)


def pad8(n):
    return n + (-n) % 8


# ---- inputs -----------------------------------------------------------------------------------------------------------------------------
def random_layer(N, K, gen):
    W = torch.randn(N, K, generator=gen) / K ** 0.5 * (torch.rand(N, K, generator=gen) < 0.6).float()
    return W, torch.rand(N, generator=gen) * 2 - 1


def random_net(widths, B, seed):
    gen = torch.Generator().manual_seed(seed)
    Ws, bs = zip(*[random_layer(widths[l + 1], widths[l], gen) for l in range(len(widths) - 1)])
    return list(Ws), list(bs), 2 * torch.randn(B, widths[0], generator=gen)


def exact_weight(N, K, r):
    S = -(-K // 32)
    n = torch.arange(N)
    k1 = 32 * ((n // 16 + r) % S) + 2 * (n % 16)
    W = torch.zeros(N, K)
    for k, sign in ((k1, 1 - 2 * ((n + r) % 2)), (k1 + 1, 1 - 2 * ((n // 3) % 2))):
        ok = k < K
        W[n[ok], k[ok]] = sign[ok].float()
    return W


def exact_net(widths, B, seed, r):
    gen = torch.Generator().manual_seed(seed)
    Ws = [exact_weight(widths[l + 1], widths[l], r) for l in range(len(widths) - 1)]
    bs = [torch.randint(-2, 3, (widths[l + 1],), generator=gen).float() for l in range(len(widths) - 1)]
    return Ws, bs, torch.randint(-8, 9, (B, widths[0]), generator=gen).float()


# ---- part 1: made_fused through umnn_made_mlp_forward_ex --------------------------------------------------------------------------------
# B: an int, or "thr" / "thr-1" (fused_threshold of the device).  name256: the kernel on 256 CUs.  shifts: exact nets run r = 0 .. shifts-1.
def _fused(id, widths, B, kind="random", shifts=1, name256=FUSED_NAMES[0], seed=0):
    return dict(id=id, widths=widths, B=B, kind=kind, shifts=shifts, name256=name256, seed=seed)


FUSED = [
    _fused("d1-1x1-B1", [1, 1], 1),
    _fused("d1-31x17-B15", [31, 17], 15),
    _fused("d1-512x1025-B16", [512, 1025], 16),                       # three output passes
    _fused("d1-33x37-B65", [33, 37], 65),
    _fused("d2-32-15-513-B17", [32, 15, 513], 17),                    # two passes, one tile in the second
    _fused("d2-63-512-512-B63", [63, 512, 512], 63),
    _fused("d3-33-16-17-1-B63", [33, 16, 17, 1], 63, seed=4),                 # 16: fewer tiles than waves
    _fused("d3-63-48-100-512-B64", [63, 48, 100, 512], 64),           # 48: odd tile count, the zeroed operand half
    _fused("d3-512-500-512-513-B65", [512, 500, 512, 513], 65),
    _fused("d3-1-1-33-17-B17", [1, 1, 33, 17], 17),
    _fused("d8-narrow-B15", [31, 17, 48, 33, 16, 100, 15, 37, 1025], 15),
    _fused("d8-wide-B16", [32, 512, 500, 100, 48, 33, 17, 16, 17], 16, seed=0),
    _fused("d3-33-48-17-17-Bthr-1", [33, 48, 17, 17], "thr-1", seed=2),
    _fused("d3-33-48-17-17-Bthr", [33, 48, 17, 17], "thr", name256=FUSED_NAMES[1], seed=2),
    _fused("x-d4-63-48-100-33-17-B17", [63, 48, 100, 33, 17], 17, "exact", 4),
    _fused("x-d2-512-512-513-B16", [512, 512, 513], 16, "exact", 16),
    _fused("x-d8-B65", [33, 17, 48, 33, 16, 100, 15, 64, 513], 65, "exact", 4),
    _fused("x-d2-33-48-17-Bthr", [33, 48, 17], "thr", "exact", 2, FUSED_NAMES[1]),
]
MODE2_WIDTHS = (1, 17, 37, 512)


def fused_B(c, cus):
    return {"thr": fused_threshold(cus), "thr-1": fused_threshold(cus) - 1}.get(c["B"], c["B"])


def fused_inputs(c, cus, r=0):
    """(Ws, bs, x) of a fused case on the CPU."""
    seed = c["seed"]            # (chosen per net: narrow output layers sit near the 1e-5 input condition, see the CPU test)
    return (exact_net(c["widths"], fused_B(c, cus), seed, r) if c["kind"] == "exact" else random_net(c["widths"], fused_B(c, cus), seed))


# ---- part 2: made_linear through umnn_made_linear_forward -------------------------------------------------------------------------------
LINEAR_B = 83                                                   # RT = 4: two row groups, the second with 19 rows
LINEAR_KS = (1, 31, 32, 33, 255, 256, 257, 512)
LINEAR_NS = (1, 17, 64, 1000)
# (row_tiles, feature_groups, name) at N = 1000: the nine variants, TG = 21 and 63 at TPC=2, and G > T
LINEAR_FORCED = [(rt, fg, linear_name(rt, tpc, (8 if rt == 4 or tpc == 2 else 16), nw))
                 for rt in (1, 2, 4) for fg, tpc, nw in ((16, 1, 4), (500, 1, 4), (8, 1, 8), (3, 2, 8), (1, 2, 8))]
# at N = 1, 17, 64 (T = 1, 2, 4) a workgroup never owns more than four tiles
LINEAR_FORCED_SMALL = [(rt, fg, linear_name(rt, 1, 8 if rt == 4 else 16, 4)) for rt in (1, 2, 4) for fg in (1, 3)]
LINEAR_AUTO_256 = linear_name(1, 1, 16, 8)                      # (0, 0) at B = 83, N = 1000 on 256 CUs: RT = 1, G = 15, TG = 5
LINEAR_EXACT_K = 257                                            # nine K-steps with a one-column last one: refills the ring at PD = 8


def linear_inputs(K):
    """(W [1000, K], b, x [LINEAR_B, K]); narrower layers take the first N rows."""
    gen = torch.Generator().manual_seed(2000 + K)
    W, b = random_layer(max(LINEAR_NS), K, gen)
    return W, b, 2 * torch.randn(LINEAR_B, K, generator=gen)


def linear_k1s(K):
    return sorted({k1 for k1 in (1, 4, K - 4, K - 1) if 1 <= k1 < K})


def linear_vec(K, K1, aligned=True):
    """Whether the launcher takes the 16-byte operand loads."""
    K1 = K if K1 is None else K1
    return aligned and K1 % 4 == 0 and (K - K1) % 4 == 0


# ---- part 3: umnn_made_split3 -----------------------------------------------------------------------------------------------------------
def split3_shapes(cus):
    """(rows, cols, relu): more pairs than the 16 * cus workgroups of 256 threads hold, so the grid-stride loop runs."""
    rows = 16 * cus + 104                                       # 4200 on 256 CUs
    return [(rows, 512, 1), (rows, 511, 0)]


# ---- part 4: umnn_made_relu_bwd_bias ----------------------------------------------------------------------------------------------------
RB_NS = (1, 3, 4, 63, 64, 255, 256, 257, 260, 1000, 1023)
RB_BS = (1, 3, 4, 5, 15, 16, 17, 63, 64, 65, 1000, 5000)
RB_SHAPES = sorted({(B, N) for N in RB_NS for B in (17, 65)} | {(B, N) for B in RB_BS for N in (64, 257)})


def rb_row_blocks(B, auto):
    return sorted({1, 7, 64, B, B + 5, auto})


def rb_inputs(B, N, kind):
    gen = torch.Generator().manual_seed(3000 + 7 * B + N)
    if kind == "exact":
        g = torch.randint(-8, 9, (B, N), generator=gen).float()
        a = torch.tensor([0.0, -0.0, 1.5, 0.25])[torch.randint(0, 4, (B, N), generator=gen)]
    else:
        g = torch.randn(B, N, generator=gen)
        a = torch.relu(torch.randn(B, N, generator=gen))
    return g, a


def rb_truth(g, a):
    """(g_y float32, column sums float64, sum_r |g_y| float64, E32) -- a = None: no ReLU behind the layer."""
    gy = g if a is None else torch.where(a > 0, g, torch.zeros_like(g))
    s64 = gy.double().sum(0)
    mag = gy.double().abs().sum(0).clamp_min(1e-300)
    e32 = float(((gy.sum(0).double() - s64).abs() / mag).max())
    return gy, s64, mag, max(e32, FLOOR)


# ---- part 5: the training glue ----------------------------------------------------------------------------------------------------------
GLUE_DS = (1, 2, 63, 64, 65, 128, 200)


def glue_Bs(d):
    """B d below, at and above 256; 1, 3, 4, 5 rows for the four-rows-per-workgroup kernels."""
    return sorted({1, 3, 4, 5, 255 // d, -(-256 // d), 257 // d, -(-257 // d)} - {0} | ({255, 256, 257} if d == 1 else set()))


def glue_inputs(B, d):
    gen = torch.Generator().manual_seed(4000 + 13 * B + d)
    r = lambda *s: torch.randn(*s, generator=gen)                        # noqa: E731
    f_x = torch.rand(B, d, generator=gen) * 2 + 0.05
    f_x.view(-1)[0::7] = 0.0
    f_x.view(-1)[3::7] = 1e-12
    return dict(g_z=r(B, d), g_lj=r(B, d), f_x=f_x, scaling=torch.rand(d, generator=gen) * 6 - 3, z=2 * r(B, d), lj=r(B, d), g_ll=r(B))


def rel_ratio(got, truth64, f32_value):
    """Per element: |got - truth| / |truth| over E32, E32 from the same formula in float32 torch (0 where truth is 0: then got must be)."""
    nz = truth64 != 0
    den = truth64.abs().clamp_min(1e-300)
    e32 = float((((f32_value.double() - truth64).abs() / den)[nz]).max()) if nz.any() else 0.0
    err = float((((got.double() - truth64).abs() / den)[nz]).max()) if nz.any() else 0.0
    assert torch.equal(got.double()[~nz], truth64[~nz])
    return err / max(e32, FLOOR)


def cotangents_truth(I, reverse_z):
    """(gF, g_fx) in float64 and in float32 torch."""
    gz = I["g_z"].flip(1) if reverse_z else I["g_z"]
    den32 = I["f_x"] + torch.tensor(1e-10, dtype=torch.float32)
    return (torch.exp(I["scaling"].double()) * gz.double(), I["g_lj"].double() / den32.double(),
            torch.exp(I["scaling"]) * gz, I["g_lj"] / den32)


LOG_2PI = 1.8378770664093453


def ll_truth(z, lj):
    """(ll float64, sum of the absolute summands per row, ll in float32 torch).  The summands are log_jac_i and (log 2 pi + z_i^2) / 2:
    the rounding error of every term scales with those, not with their difference."""
    ll = (lj.double() - 0.5 * (LOG_2PI + z.double() ** 2)).sum(1)
    mag = (lj.double().abs() + 0.5 * (LOG_2PI + z.double() ** 2)).sum(1)
    return ll, mag, (lj - 0.5 * (LOG_2PI + z * z)).sum(1)


def ll_probes(d):
    """(z, lj, want): rows of zeros except one log_jac of 1024 at column e in {0, 63, 64, d - 1}."""
    es = sorted({e for e in (0, 63, 64, d - 1) if e < d})
    lj = torch.zeros(len(es), d)
    for i, e in enumerate(es):
        lj[i, e] = 1024.0
    z = torch.zeros(len(es), d)
    return z, lj, ll_truth(z, lj)[0]


# ---- ctypes helpers ---------------------------------------------------------------------------------------------------------------------
def made_net(widths, W_ptrs, b_ptrs, n_layers=None):
    """struct umnn_made_net of the first n_layers layers."""
    net = _lib.MadeNet()
    L = len(widths) - 1 if n_layers is None else n_layers
    net.n_layers = L
    for i, w in enumerate(widths[:_lib.MADE_MAX_LAYERS + 1]):
        net.widths[i] = w
    for l in range(min(L, _lib.MADE_MAX_LAYERS, len(W_ptrs))):
        net.W[l], net.b[l] = W_ptrs[l], b_ptrs[l]
    return net


def ptr(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def as_numpy64(ts):
    return [t.double().numpy() for t in ts]
