"""Case table, inputs, float64 truth and bounds of the multi-output quadrature coverage tests: tests/test_multi_coverage_cpu.py (the
plan arithmetic, completeness, the kink guard, the truth pin and the size of the bounds, no GPU) and
tests/test_gpu_multi_coverage.py (every case on the device, through umnn_cc_forward_multi / umnn_cc_backward_multi themselves).

Names.  Every expected family, name, pass count and waves-per-workgroup below was derived by hand from multi_plan and multi_passes
of csrc/cc_multi.hip, not read back from the library (which has no entry that would tell):
  * a hidden layer of width H has ceil((H + 1) / 16) tiles and ceil((H + 1) / 4) K-steps (the constant one rides as feature H).
    The family (T, KS) is the first of (2,8), (4,13), (4,16), (7,26), (8,32) that holds the widest layer: H <= 31, <= 51, <= 63,
    <= 103 (104 + 1 features are 27 K-steps), <= 127.  The forward is cc_fwd_multi<T,KS,P>, P = 2 from 2 x 4 x CUs tiles of 16.
  * backward passes over nimg = hidden layers - 1 images, the first the EDGE pass:
      T <= 4:            <NACC=3,EDGE=1,OUTW=1>, then <NACC=3,EDGE=0,OUTW=0> per further three images (five to seven layers: two);
      T = 7, nimg >= 2:  <NACC=1,EDGE=1,OUTW=0>, then <NACC=1,EDGE=0,OUTW=1> for image 2, <NACC=1,EDGE=0,OUTW=0> for each after it;
      T = 7, nimg <= 1 and T = 8: <NACC=0,EDGE=1,OUTW=1>, then <NACC=1,EDGE=0,OUTW=0> per image.
    Without d_theta only the first pass runs, so `first` is what a dtheta = NULL call notes and `last` what a full call notes.
    <T=7,KS=26,NACC=1,EDGE=1,OUTW=0> is always followed by another pass in a full call: it is a `first` only.
  * LDS of the backward, in floats: a row-major image has 4 KS rows of ld columns, ld = the smallest value >= 4 KS that is 14 or 18
    modulo 32 (46, 78, 78, 110, 142); the output image 16 rows; 16 T for the first layer's x-column; per wave (nacc + 1) T 256 + 256
    with nacc = 3 for T <= 4, else 1.  Four waves per workgroup, halved while the sum exceeds 40960 floats (160 KiB):
      (4,13): 4056 nimg + 1248 + 64 + 4 x 4352: six images (seven hidden layers) are 43056 -> two waves, 34352;
      (4,16): 4992 nimg + 1248 + 64 + 4 x 4352: five images (six hidden layers) are 43680 -> two waves, 34976;
      (7,26): 11440 nimg + 1760 + 112 + 4 x 3840: three images (four hidden layers) are 51552 -> one wave, 40032 = 160128 bytes;
      (8,32): 18176 nimg + 2272 + 128 + 4 x 4352: one image fits (37984), two do not even with one wave (43104): no kernel.

Inputs.  As tests/_bwd_coverage_cases.py: IntegrandNetwork(d, 1 + E, hidden, K) default-initialised from a seed of its own,
parameters x 1.7; rows drawn in float64 on the CPU from a fixed seed, rounded to float32, and kept only when the smallest |z| /
(sum_k |W_jk a_k| + |b_j|) over every hidden unit, at all n + 1 nodes and at x and x0, of each of the row's d integrals is at least
GUARD = 1e-5 (`margin_rows` of that file).  At most half of the drawn rows of any case may be rejected (asserted on the CPU).  The
forward-only launches of part 4 draw without rejection: values are continuous across a kink.

Truth and bounds.  `quadrature` evaluates the B d row problem in torch on the float32-rounded weights, inputs and Clenshaw-Curtis
tables: F, f(x), f(x0), and by autograd d_h and d_theta of sum(F g); d_x = sum_k g_k f_k(x), d_x0 = -sum_k g_k f_k(x0) (the Leibniz
terms, f itself also under inv_f, as the operator defines them).  In float64 it is the truth, in float32 the same arithmetic at the
kernels' precision: e32 = the error of the float32 run against the float64 one (U.rel_err for F, f_x, f_x0, d_x, d_x0; U.scaled_err
for d_h and each parameter tensor of d_theta), E32 = max(e32, 2^-22).  A kernel output must be within M x E32 of the truth, never
above the 1e-5 of tests/_multi_output_cases.py: M = 8 for values (the fp32 figure of tests/_fwd_coverage_cases.py) and M_GRAD for
gradients (profiles/multi_coverage/README.md)."""
import types

import numpy as np
import torch

from tests import _util as U
from tests._bwd_coverage_cases import margin_rows
from tests._multi_output_cases import TOL as OUTER
from umnn_amd import _lib
from umnn_amd.quadrature import compute_cc_weights

ELU, SIGMOID = _lib.OUT_ELU_PLUS_ONE, _lib.OUT_SIGMOID
LEAKY, RELU = _lib.ACT_LEAKY_RELU, _lib.ACT_RELU
GUARD = 1e-5
REJECT_CAP = 0.5
FLOOR = 2.0 ** -22
M_VALUE = 8.0
M_GRAD = 8.0
VALUES, GRADS = ("F", "fx", "fx0"), ("dx0", "dx", "dh", "dtheta")

CASES = []


def fwd_name(T, KS, P=1):
    return f"cc_fwd_multi<T={T},KS={KS},P={P}>"


def bwd_name(T, KS, nacc, edge, outw):
    return f"cc_bwd_multi<T={T},KS={KS},NACC={nacc},EDGE={edge},OUTW={outw}>"


def case(id, part, fam, hid, passes, last, first, wpb=4, K=5, B=37, d=3, E=4, n=6, act=LEAKY, out_act=ELU, x0=True, inv_f=False):
    """fam: (T, KS); last / first: (nacc, edge, outw) of the last pass of a full call and of the only pass of a dtheta = NULL call"""
    c = dict(id=id, part=part, fam=fam, hid=list(hid), passes=passes, fwd=fwd_name(*fam), last=bwd_name(*fam, *last), first=bwd_name(*fam, *first),
             wpb=wpb, K=K, B=B, d=d, E=E, n=n, act=act, out_act=out_act, x0=x0, inv_f=inv_f)
    assert all(o["id"] != id for o in CASES), id
    CASES.append(c)
    return c


def tag(hid):
    return "x".join(map(str, hid))


# ---- part 1: every family and every backward variant by name; B = 37, d = 3: 111 integrals in 7 tiles, the last of 15 lanes --------
E3, R3 = (3, 1, 1), (3, 0, 0)                      # T <= 4: the EDGE pass and the pass of images 4..6
for _fam, _nets in (((2, 8), ([15], [16], [31], [20, 31, 9], [31] * 5, [16, 31, 15, 20, 8, 31])),
                    ((4, 13), ([32], [51], [51, 40, 33], [51] * 5, [51, 32, 48, 40, 36, 51], [40] * 7)),
                    ((4, 16), ([52], [63], [63, 52, 60], [63] * 5, [52, 63, 56, 60, 63, 55]))):
    for _hid in _nets:
        _two = len(_hid) >= 5
        _wpb = 2 if (_fam == (4, 13) and len(_hid) == 7) or (_fam == (4, 16) and len(_hid) == 6) else 4
        case(f"p1-{tag(_hid)}", 1, _fam, _hid, 2 if _two else 1, R3 if _two else E3, E3, wpb=_wpb)
case("p1-64", 1, (7, 26), [64], 1, (0, 1, 1), (0, 1, 1))
case("p1-103", 1, (7, 26), [103], 1, (0, 1, 1), (0, 1, 1))
case("p1-103x64", 1, (7, 26), [103, 64], 2, (1, 0, 0), (0, 1, 1))
case("p1-80x103x70", 1, (7, 26), [80, 103, 70], 2, (1, 0, 1), (1, 1, 0))
case("p1-103x4", 1, (7, 26), [103] * 4, 3, (1, 0, 0), (1, 1, 0), wpb=1)
case("p1-104", 1, (8, 32), [104], 1, (0, 1, 1), (0, 1, 1))
case("p1-127", 1, (8, 32), [127], 1, (0, 1, 1), (0, 1, 1))
case("p1-127x104", 1, (8, 32), [127, 104], 2, (1, 0, 0), (0, 1, 1))
case("p1-104x127", 1, (8, 32), [104, 127], 2, (1, 0, 0), (0, 1, 1))

# ---- part 2: the flags on one representative per family (the part-1 case of the same net has x0, LeakyReLU, ELU + 1, K = 5) --------
REPS = {(2, 8): ([20, 31, 9], 1, E3, E3), (4, 13): ([51, 40, 33], 1, E3, E3), (4, 16): ([63, 52, 60], 1, E3, E3),
        (7, 26): ([80, 103, 70], 2, (1, 0, 1), (1, 1, 0)), (8, 32): ([127, 104], 2, (1, 0, 0), (0, 1, 1))}
FLAGS = [("no-x0", dict(x0=False, K=2)), ("inv_f", dict(inv_f=True, K=3)), ("relu", dict(act=RELU, K=4)), ("sigmoid", dict(out_act=SIGMOID, K=13)),
         ("K16", dict(K=16))]
REP_CASES, FLAG_CASES = {}, {}
for _fam, (_hid, _passes, _last, _first) in REPS.items():
    REP_CASES[_fam] = next(c for c in CASES if c["hid"] == _hid and c["part"] == 1)
    for _flag, _kw in FLAGS:
        FLAG_CASES[_fam, _flag] = case(f"p2-{tag(_hid)}-{_flag}", 2, _fam, _hid, _passes, _last, _first, **_kw)
NEED_MASKS = [(a, b, c, e) for a in (0, 1) for b in (0, 1) for c in (0, 1) for e in (0, 1)]      # (dx0, dx, dh, dtheta) asked for

# ---- part 3: count edges, on the two-layer 12-9 net of the (2,8) family (few units: the rejection cap holds at d = 63 and n = 50) ---
EDGE_NET = [12, 9]
# B d = 1, 15, 16, 17, 33, 129, 153, 315; then 417, 501 and 513 integrals: 27, 32 and 33 tiles in 7, 8 and 9 forward workgroups of four
COUNT_SHAPES = [(1, 1), (15, 1), (16, 1), (17, 1), (33, 1), (43, 3), (9, 17), (5, 63), (139, 3), (167, 3), (171, 3)]
COUNT_BLOCKS = {(139, 3): 7, (167, 3): 8, (171, 3): 9}
COUNT_CASES = [case(f"p3-count-{_B}x{_d}", 3, (2, 8), EDGE_NET, 1, E3, E3, B=_B, d=_d) for _B, _d in COUNT_SHAPES]
NODE_CASES = [case(f"p3-n{_n}", 3, (2, 8), EDGE_NET, 1, E3, E3, n=_n) for _n in (1, 2, 3, 50)]
EMBED_CASES = [case(f"p3-E{_E}", 3, (2, 8), EDGE_NET, 1, E3, E3, E=_E) for _E in (0, 1, 5, 30)]

BY_ID = {c["id"]: c for c in CASES}

# ---- part 4: large launches, n = 2 -------------------------------------------------------------------------------------------------
LARGE_NET = [20, 31, 9]
CHUNK_INTEGRALS = 8192          # 512 tiles: P = 1 (P = 2 from 8 cus tiles), one group per wave (4 cus waves), 128 < 2 cus so qpb = 16, from 64 CUs on


def large_shapes(cus):
    """(A, B): A = 2 x 4 x cus + 3 tiles, the last of five lanes, d = 1 -- P = 2 with an odd tile count, waves of two and of three
    groups (cus workgroups of four waves), NI / 64 >= 2 cus so qpb = 64, ceil(NI / 64) dw0 parts.  B = 65538 integrals with d = 3:
    1024 dw0 parts of per = 65."""
    tiles = 2 * 4 * cus + 3
    return dict(id="p4-A", B=16 * (tiles - 1) + 5, d=1), dict(id="p4-B", B=21846, d=3)


def large_case(shape, fam=(2, 8), hid=LARGE_NET):
    rep = REPS[fam]
    return dict(id=f"{shape['id']}-{tag(hid)}", part=4, fam=fam, hid=list(hid), passes=rep[1], fwd=fwd_name(*fam, 2), last=bwd_name(*fam, *rep[2]),
                first=bwd_name(*fam, *rep[3]), wpb=4, K=5, B=shape["B"], d=shape["d"], E=4, n=2, act=LEAKY, out_act=ELU, x0=True, inv_f=False)


# ---- the rule, restated (tests/test_multi_coverage_cpu.py holds the table to it) --------------------------------------------------------
FAMILIES = [(2, 8), (4, 13), (4, 16), (7, 26), (8, 32)]
LDS_FLOATS = 160 * 1024 // 4


def family_of(hid):
    tiles, ks = max((H + 1 + 15) // 16 for H in hid), max((H + 1 + 3) // 4 for H in hid)
    return next(((T, KS) for T, KS in FAMILIES if tiles <= T and ks <= KS), None)


def multi_ld(cols):
    ld = cols
    while ld % 32 not in (14, 18):
        ld += 1
    return ld


def bwd_lds_floats(fam, nimg, waves):
    T, KS = fam
    ld = multi_ld(4 * KS)
    return nimg * 4 * KS * ld + 16 * ld + 16 * T + waves * (((3 if T <= 4 else 1) + 1) * T * 256 + 256)


def fwd_lds_floats(fam, nimg):
    return (nimg * fam[0] + 1) * fam[1] * 64


def wpb_of(fam, nimg):
    """waves per workgroup of the backward, or 0 when even one wave does not fit"""
    wpb = 4
    while wpb > 1 and bwd_lds_floats(fam, nimg, wpb) > LDS_FLOATS:
        wpb //= 2
    return wpb if bwd_lds_floats(fam, nimg, wpb) <= LDS_FLOATS else 0


def passes_of(fam, nimg, need_theta=True):
    """[(nacc, edge, outw)] of the passes of a backward over nimg hidden images"""
    T = fam[0]
    if T <= 4:
        return [(3, 1, 1)] + ([(3, 0, 0)] * len(range(4, nimg + 1, 3)) if need_theta else [])
    if T == 7 and nimg >= 2:
        return [(1, 1, 0)] + ([(1, 0, 1 if l == 2 else 0) for l in range(2, nimg + 1)] if need_theta else [])
    return [(0, 1, 1)] + ([(1, 0, 0)] * nimg if need_theta else [])


def n_params(c):
    w = [1 + c["E"]] + c["hid"] + [c["K"]]
    return sum(w[i] * w[i + 1] + w[i + 1] for i in range(len(w) - 1))


def workspace_bytes(c, NI, cus=256):
    """[d_theta slices: 4 waves x cus][dc: NI x H1][first-layer partials: min(ceil(NI / 64), 1024) x H1 (E + 1)], each rounded to 256"""
    up = lambda v: (v + 255) & ~255
    H1 = c["hid"][0]
    return up(up(up(cus * 4 * n_params(c) * 4) + NI * H1 * 4) + min((NI + 63) // 64, 1024) * H1 * (c["E"] + 1) * 4)


def desc(c, ptr=0x1000):
    """struct umnn_mlp of a case with placeholder pointers (the plan reads widths and activations only)"""
    widths = [1 + c["E"]] + c["hid"] + [c["K"]]
    m = _lib.MlpDesc()
    m.n_linear = len(widths) - 1
    for i, w in enumerate(widths):
        m.widths[i] = w
    for l in range(m.n_linear):
        m.W[l], m.b[l] = ptr, ptr
    m.hidden_act, m.out_act = c["act"], c["out_act"]
    return m


# ---- inputs -----------------------------------------------------------------------------------------------------------------------
def make_net(c):
    """IntegrandNetwork of the case on the CPU, default-initialised from a seed of its own, parameters x 1.7."""
    import umnn_amd
    with torch.random.fork_rng(devices=[]):
        torch.manual_seed(3000 + 7 * sum(c["hid"]) + 31 * len(c["hid"]) + c["E"] + 101 * c["K"])
        net = umnn_amd.IntegrandNetwork(c["d"], 1 + c["E"], list(c["hid"]), c["K"], act_func="Sigmoid" if c["out_act"] == SIGMOID else "ELU")
    if c["act"] == RELU:
        for i in range(1, 2 * len(c["hid"]), 2):
            net.net[i] = torch.nn.ReLU()
    with torch.no_grad():
        for p in net.parameters():
            p.mul_(1.7)
    return net


def _input_key(c):
    return (tuple(c["hid"]), c["K"], c["act"], c["out_act"], c["B"], c["d"], c["E"], c["n"], c["x0"])


_INPUTS, _TRUTH = {}, {}


def inputs(c, guard=GUARD):
    """-> namespace(net, x0, x [B, d], h [B, E d] (index e d + i), g [B, d, K]: float64 CPU tensors holding float32 values, x0 None
    where the case passes none; reject: the fraction of drawn rows rejected; margin: the smallest margin of a kept row).  guard = 0
    keeps every row (the forward-only launches).  Computed once per distinct input set and shared; nothing in it is modified."""
    key = _input_key(c) + (guard,)
    if key in _INPUTS:
        return _INPUTS[key]
    net = make_net(c)
    B, d, E, n, K = c["B"], c["d"], c["E"], c["n"], c["K"]
    gen = torch.Generator().manual_seed(6007 + 131 * B + 17 * d + E + 1009 * n + 7 * K)
    kept, margins, drawn, used = [], [], 0, 0
    while used < B:                                   # rows are examined in the order drawn, block by block, up to the B-th kept one
        R = 2 * B + 32
        blk = [(torch.randn(R, w, generator=gen, dtype=torch.float64) * sc).float().double()
               for w, sc in ((d, 2.0), (d, 0.3), (E * d, 1.0), (d * K, 1.0))]
        x, x0, h = blk[0], (blk[1] if c["x0"] else torch.zeros_like(blk[1])), blk[2]
        m = margin_rows(net, x0.numpy(), x.numpy(), h.numpy(), n) if guard > 0 else np.full(R, np.inf)
        ok = np.flatnonzero(m >= guard)[:B - used]
        drawn += R if used + len(ok) < B else int(ok[-1]) + 1
        used += len(ok)
        kept.append([t[ok] for t in blk])
        margins.append(m[ok])
    x, x0, h, g = (torch.cat([k[i] for k in kept]) for i in range(4))
    out = types.SimpleNamespace(net=net, x=x, x0=x0 if c["x0"] else None, h=h, g=g.view(B, d, K), reject=1.0 - B / drawn,
                                margin=float(np.concatenate(margins).min()))
    _INPUTS[key] = out
    return out


def rows_of(x, h, d):
    """[B, d], [B, E d] -> the B d row problem: x [B d], h [B d, E] (what test_abi_with_three_dimensions does)"""
    B = x.shape[0]
    return x.reshape(B * d), h.view(B, -1, d).transpose(1, 2).reshape(B * d, -1)


# ---- truth ------------------------------------------------------------------------------------------------------------------------
def quadrature(f, params, x0, x, h, g, n, inv_f=False, dtype=torch.float64, chunk=4096, grads=True):
    """The row problem in `dtype`: f(rows [R, 1 + E]) -> [R, K] built on `params` (tensors of that dtype), x0 / x [R] (x0 None: zeros),
    h [R, E], g [R, K] -> namespace of numpy arrays F, fx, fx0 [R, K]; dx0, dx [R]; dh [R, E]; dtheta: one array per entry of params.
    F = (x - x0) / 2 sum_j w_j f(t_j) (1 / f under inv_f), t_j = x0 + (x - x0)(s_j + 1) / 2 on the float32-rounded tables."""
    w, s = (t.reshape(-1).to(dtype) for t in compute_cc_weights(n))
    x, h, g = x.to(dtype), h.to(dtype), g.to(dtype)
    x0 = torch.zeros_like(x) if x0 is None else x0.to(dtype)
    acc = [torch.zeros_like(p) for p in params]
    out = {k: [] for k in ("F", "fx", "fx0", "dx0", "dx", "dh")}
    for lo in range(0, x.shape[0], chunk):
        xa, x0a, ga = x[lo:lo + chunk], x0[lo:lo + chunk], g[lo:lo + chunk]
        ha = h[lo:lo + chunk].detach().requires_grad_(grads)
        r = xa.shape[0]
        t = x0a[:, None] + (xa - x0a)[:, None] * (s[None, :] + 1) / 2
        rows = torch.cat((t[:, :, None], ha[:, None, :].expand(r, n + 1, ha.shape[1])), 2).reshape(r * (n + 1), -1)
        v = f(rows).view(r, n + 1, -1)
        F = ((1 / v if inv_f else v) * w[None, :, None]).sum(1) * ((xa - x0a) / 2)[:, None]
        if grads:
            gr = torch.autograd.grad((F * ga).sum(), list(params) + ([ha] if ha.shape[1] else []))
            for a, b in zip(acc, gr):
                a += b
            out["dh"].append(gr[len(params)] if ha.shape[1] else torch.zeros_like(ha))
        with torch.no_grad():
            fx, fx0 = f(torch.cat((xa[:, None], ha), 1)), f(torch.cat((x0a[:, None], ha), 1))
        out["F"].append(F.detach()); out["fx"].append(fx); out["fx0"].append(fx0)
        out["dx"].append((ga * fx).sum(1)); out["dx0"].append(-(ga * fx0).sum(1))
    res = {k: torch.cat(v).detach().numpy() for k, v in out.items() if v}
    return types.SimpleNamespace(dtheta=[a.numpy() for a in acc] if grads else None, **res)


def case_quadrature(c, i, dtype, rows=None, grads=True):
    """`quadrature` of a case's inputs `i` (all rows, or the integrals `rows`) on its float32-rounded weights"""
    import copy
    seq = copy.deepcopy(i.net.net).to(dtype)
    x, h = rows_of(i.x, i.h, c["d"])
    x0 = None if i.x0 is None else i.x0.reshape(-1)
    g = i.g.reshape(-1, c["K"])
    if rows is not None:
        x, h, g, x0 = x[rows], h[rows], g[rows], (None if x0 is None else x0[rows])
    return quadrature(seq, list(seq.parameters()), x0, x, h, g, c["n"], c["inv_f"], dtype, grads=grads)


def errors(got, ref):
    """{output: error of `got` against `ref`} by the criterion of each output; dtheta: a list, one per parameter tensor"""
    e = {k: U.rel_err(getattr(got, k), getattr(ref, k)) for k in VALUES + ("dx0", "dx") if getattr(got, k, None) is not None}
    if getattr(got, "dh", None) is not None:
        e["dh"] = U.scaled_err(got.dh, ref.dh)
    if getattr(got, "dtheta", None) is not None:
        e["dtheta"] = [U.scaled_err(a, b) for a, b in zip(got.dtheta, ref.dtheta)]
    return e


def truth(c, guard=GUARD, rows=None, grads=True):
    """-> namespace(t: the float64 truth, t32: the float32 run, E32: {output: max(error of t32 against t, 2^-22)}, dtheta a list).
    Computed once per distinct (input set, inv_f) and shared; callers must not modify it."""
    key = _input_key(c) + (c["inv_f"], guard, None if rows is None else (int(rows[0]), int(rows[-1]), len(rows)), grads)
    if key not in _TRUTH:
        i = inputs(c, guard)
        t, t32 = (case_quadrature(c, i, dt, rows, grads) for dt in (torch.float64, torch.float32))
        E32 = {k: ([max(v, FLOOR) for v in e] if isinstance(e, list) else max(e, FLOOR)) for k, e in errors(t32, t).items()}
        _TRUTH[key] = types.SimpleNamespace(t=t, t32=t32, E32=E32)
    return _TRUTH[key]


def bound(E32, name):
    """the rel_err / scaled_err bound of one output (one parameter tensor of dtheta): M x E32, never above 1e-5"""
    return min((M_VALUE if name in VALUES else M_GRAD) * E32, OUTER)
