"""Case table, inputs, float64 truth and bounds of the quadrature-forward coverage tests: tests/test_forward_coverage_cpu.py (plan
fields, completeness, the truth pin and the size of the bounds, no GPU) and tests/test_gpu_forward_coverage.py (every case on the
device).

Names.  Every expected name, P, ns and waves below was derived by hand from csrc/cc_fwd_plan.h for a device of 256 CUs, not read back
from the library:
  * a hidden layer of width H has (H + 16) // 16 tiles and (H + 4) // 4 K-steps of four (the bias rides as feature H).  LIVE = the
    common K-step count when a variant has it (13: widths 48..51; 26: 100..103), else 0.
  * tiles = ceil(B d / 16).  P = 1 below 8192 tiles; the node range is split ns = 4 ways up to 1024 tiles (512 for the uniform wide and
    the wide-first nets), never into more parts than the n + 1 nodes (then 1) -- fwd_p and fwd_ns force either, fwd_ns under the same
    node limit.  The base shape B = 37, d = 3 is 111 integrals in 7 tiles: ns = 4 unforced at n = 20.
  * f16x3 (default): cc_fwd_f16 with the bf16 build queued (fallback = 1) -- cc_fwd_bf16 outright when F aliases an input; bf16x3:
    cc_fwd_bf16 on two pieces; bf16x6: three; fp32, or what no piece build serves: cc_fwd.
  * two pieces: every hidden layer of the same 5..8 tiles and P = 1: T=5..8 exact, eight waves per workgroup when two workgroups of
    images (+ 1 KiB each) exceed 160 KiB, an image being t_out x (t_in / 2 K-steps of 1 KiB + a half one for odd t_in) x 2 pieces
    (70x5: 4 x 25 KiB, 90x4: 3 x 36, 100x3 / 110x3: 2 x 49, 120x3: 2 x 64; two layers are one image: four waves).  First layer of
    5..8 tiles over layers of <= 4 and P = 1: the wide-first kernels, LIVE=13 when the rest is 48..51 wide.  Else the tile bucket
    2 / 4 / 8: EXACT when every layer fills it; inexact nets of 3..4 tiles are zero-padded to EXACT=1, T=4, LIVE=0 unless fwd_pad = 0;
    EXACT, T=4, P = 2 runs the PIPE variant unless fwd_pipe = 0.  No exact variant: the generic one of the bucket (EXACT=0, LIVE=0);
    fwd_p = 2 on a wide or wide-first net is the generic T=8 one.  Three pieces: T=4 exact or generic T=2 / T=4, never padded.
    fwd_pipe = 2 on the bf16 build, two pieces, LIVE=13: the 32x32x16 kernel, P = 2, ns = 1 always.
  * fp32: TAIL=1 for widths 50 (fwd_tail = 0 and width 51: TAIL=0), KS=26 for widths 100..103, else generic T = 2 / 4 / 8.

Inputs.  IntegrandNetwork default-initialised, parameters x 1.7; x ~ 2 N(0,1), x0 ~ 0.3 N(0,1), h ~ N(0,1), scaling ~ 0.1 N(0,1),
log_jac_in ~ N(0,1), fixed seeds on the CPU; bf16-storage cases round them to bf16 first.  E = 4: no family needs a wide input (the
first layer is the same hoisted fp32 term everywhere); the flag E=30 of part 2 runs eight embedding K-steps with a partial last one.

Truth and bounds.  reference() evaluates the quadrature in float64 (torch) on the float32-rounded weights, inputs and
Clenshaw-Curtis tables, and the reference's own arithmetic (oracle.cc_oracle on float32 arrays); e32 = U.rel_err of the latter
against the former, E32 = max(e32, 2^-22) (two fp32 ulps at magnitude 1, which is what rel_err normalises to).  A kernel output
must be within M x E32 of the truth: M = 8 for fp32, bf16x6 and f16x3 (two fp16 pieces carry 22 of 24 significand bits: 4; another
summation order and v_exp_f32: 2), M = 64 for bf16x3 (include/umnn_cc.h: 6e-6 against 4e-7 is 15; 4 for other shapes)."""
import copy
import types

import numpy as np
import torch

from oracle import cc_oracle as O
from tests import _util as U
from tests._fwd_plan_cases import bf16, desc, f16      # noqa: F401  (desc: struct umnn_mlp of a case; re-exported)
from umnn_amd import _lib
from umnn_amd.quadrature import compute_cc_weights

ELU, SIGMOID = _lib.OUT_ELU_PLUS_ONE, _lib.OUT_SIGMOID
LEAKY, RELU = _lib.ACT_LEAKY_RELU, _lib.ACT_RELU
PREC = {k: dict(fwd_precision=v) for k, v in _lib.PRECISIONS.items()}
FLOOR = 2.0 ** -22
OUTER = 1e-4            # the bound of every older forward parity test: kept as an outer bound
M_FP32_LEVEL, M_BF16X3 = 8.0, 64.0
P32 = "cc_fwd_bf16<32x32x16,PARTS=2,P=2,EXACT=1,LIVE=26,PIPE32>"
N50, N60, PADDED = [50] * 4, [60] * 4, [48, 60, 36, 50]

CASES = []


def case(id, part, family, hid, name, pieces=2, P=1, ns=4, waves=4, fallback=0, B=37, d=3, E=4, n=20, act=LEAKY, out_act=ELU, x0=True,
         inv_f=False, x_bf16=False, h_bf16=False, alias=False, null_fx=False, **options):
    c = dict(id=id, part=part, family=family, hid=list(hid), name=name, pieces=pieces, P=P, ns=ns, waves=waves, fallback=fallback, B=B, d=d,
             E=E, n=n, act=act, out_act=out_act, x0=x0, inv_f=inv_f, x_bf16=x_bf16, h_bf16=h_bf16, alias=alias, null_fx=null_fx,
             options=options)
    assert all(o["id"] != id for o in CASES), id
    CASES.append(c)
    return c


def tag(hid):
    return "x".join(map(str, hid))


def mode(c):
    """the arithmetic a case runs: fp32 | bf16x6 | f16x3 | bf16x3 (an aliased f16x3 launch runs the bf16x3 build)"""
    m = next(k for k, v in _lib.PRECISIONS.items() if v == c["options"].get("fwd_precision", _lib.PRECISIONS["f16x3"]))
    if c["pieces"] == 0:
        return "fp32"
    return "bf16x3" if (m == "f16x3" and c["alias"]) else m


def M(c):
    return M_BF16X3 if mode(c) == "bf16x3" else M_FP32_LEVEL


# ---- the 81 kernels, one row each: (key, net, name, pieces, P, waves, fallback, options) -------------------------------------------
WIDE_FIRST_W1 = {5: 70, 6: 90, 7: 100, 8: 120}
VARIANTS = []


def _v(key, hid, name, pieces=2, P=1, waves=4, fallback=0, **options):
    VARIANTS.append((key, list(hid), name, pieces, P, waves, fallback, options))


def _two_pieces(pre, stem, fallback, prec):
    body = "T={T},PARTS=2,P={P},EXACT={ex},LIVE={live}"
    v = lambda key, hid, T, P, ex, live, sfx="", waves=4, **o: _v(f"{pre}-{key}", hid, stem(body.format(T=T, P=P, ex=ex, live=live) + sfx),
                                                                   P=P, waves=waves, fallback=fallback, **prec, **o)
    v("pipe-live13", N50, 4, 2, 1, 13, ",PIPE", fwd_p=2)
    v("pipe-live0", N60, 4, 2, 1, 0, ",PIPE", fwd_p=2)
    v("pipe-padded", PADDED, 4, 2, 1, 0, ",PIPE", fwd_p=2)
    v("exact-live13", N50, 4, 1, 1, 13)
    v("plain-p2-live13", N50, 4, 2, 1, 13, fwd_p=2, fwd_pipe=0)
    v("exact-live0", N60, 4, 1, 1, 0)
    v("padded", PADDED, 4, 1, 1, 0)
    v("plain-p2-live0", N60, 4, 2, 1, 0, fwd_p=2, fwd_pipe=0)
    v("plain-p2-padded", PADDED, 4, 2, 1, 0, fwd_p=2, fwd_pipe=0)
    v("generic2", [20, 20], 2, 1, 0, 0)
    v("generic2-p2", [20, 20], 2, 2, 0, 0, fwd_p=2)
    v("generic4", PADDED, 4, 1, 0, 0, fwd_pad=0)
    v("generic4-p2", PADDED, 4, 2, 0, 0, fwd_pad=0, fwd_p=2)
    v("generic8", [70, 90], 8, 1, 0, 0)
    v("generic8-p2", [70, 90], 8, 2, 0, 0, fwd_p=2)
    v("t7-live26", [100, 100], 7, 1, 1, 26)
    v("t7-live0", [110, 110], 7, 1, 1, 0)
    v("t5", [70, 70], 5, 1, 1, 0)
    v("t6", [90, 90], 6, 1, 1, 0)
    v("t8", [120, 120], 8, 1, 1, 0)
    v("t7-live26-w8", [100] * 3, 7, 1, 1, 26, ",WAVES=8", waves=8)
    v("t7-live0-w8", [110] * 3, 7, 1, 1, 0, ",WAVES=8", waves=8)
    v("t5-w8", [70] * 5, 5, 1, 1, 0, ",WAVES=8", waves=8)
    v("t6-w8", [90] * 4, 6, 1, 1, 0, ",WAVES=8", waves=8)
    v("t8-w8", [120] * 3, 8, 1, 1, 0, ",WAVES=8", waves=8)
    for t1, w1 in WIDE_FIRST_W1.items():
        for live, rest in ((13, [50, 50]), (0, [60, 60])):
            _v(f"{pre}-wide-first-t{t1}-live{live}", [w1] + rest, stem(f"T1={t1},TREST=4,PARTS=2,P=1,EXACT=1,LIVE={live}"), fallback=fallback, **prec)


_two_pieces("f16", f16, 1, {})
_two_pieces("bf16", bf16, 0, PREC["bf16x3"])
for _key, _hid, _T, _ex, _live, _o in (("exact-live13", N50, 4, 1, 13, {}), ("exact-live0", N60, 4, 1, 0, {}), ("generic2", [20, 20], 2, 0, 0, {}),
                                       ("generic4", PADDED, 4, 0, 0, {})):      # (three pieces never pad)
    for _P in (1, 2):
        _v(f"bf16x6-{_key}-p{_P}", _hid, bf16(f"T={_T},PARTS=3,P={_P},EXACT={_ex},LIVE={_live}"), pieces=3, P=_P, **PREC["bf16x6"],
           **(dict(fwd_p=2) if _P == 2 else {}), **_o)
for _key, _hid, _T, _ks, _tail, _o in (("tail", N50, 4, 13, 1, {}), ("tail=0", N50, 4, 13, 0, dict(fwd_tail=0)), ("width-51", [51] * 4, 4, 13, 0, {}),
                                       ("ks26", [100] * 3, 7, 26, 0, {}), ("generic2", [20, 20], 2, 0, 0, {}), ("generic4", N60, 4, 0, 0, {}),
                                       ("generic8", [70, 90], 8, 0, 0, {})):
    for _P in (1, 2):
        _v(f"fp32-{_key}-p{_P}", _hid, f"cc_fwd<T={_T},KS={_ks},P={_P},TAIL={_tail}>", pieces=0, P=_P, **PREC["fp32"],
           **(dict(fwd_p=2) if _P == 2 else {}), **_o)
_v("p32", N50, P32, P=2, fwd_pipe=2, **PREC["bf16x3"])

# ---- part 1: every kernel by name at B = 37, d = 3, with the node range whole (fwd_ns = 1) and split by the rule (ns = 4) ---------
PART1 = {}
for _key, _hid, _name, _pieces, _P, _waves, _fb, _opt in VARIANTS:
    _auto_ns = 1 if _name == P32 else 4
    PART1[_key] = (case(f"{_key}-ns1", 1, _key, _hid, _name, _pieces, _P, 1, _waves, _fb, fwd_ns=1, **_opt),
                   case(f"{_key}-auto", 1, _key, _hid, _name, _pieces, _P, _auto_ns, _waves, _fb, **_opt))

# ---- part 2: the flags on one representative per family ----------------------------------------------------------------------------
REPS = {      # family: the key of its row of VARIANTS
    "f16-exact13": "f16-exact-live13", "f16-pipe": "f16-pipe-live13", "f16-exact0": "f16-padded", "f16-generic2": "f16-generic2",
    "f16-t7-w8": "f16-t7-live26-w8", "f16-wide-first": "f16-wide-first-t7-live13", "bf16-2": "bf16-exact-live13", "bf16-3": "bf16x6-exact-live13-p1",
    "p32": "p32", "fp32-tail": "fp32-tail-p1", "fp32-ks26": "fp32-ks26-p1", "fp32-generic": "fp32-generic2-p1",
}
_BY_KEY = {v[0]: v for v in VARIANTS}
FLAGS = [("no-x0", dict(x0=False)), ("inv_f", dict(inv_f=True)), ("relu", dict(act=RELU)), ("sigmoid", dict(out_act=SIGMOID)),
         ("null-fx", dict(null_fx=True)), ("x-bf16", dict(x_bf16=True)), ("h-bf16", dict(h_bf16=True)), ("xh-bf16", dict(x_bf16=True, h_bf16=True)),
         ("E=30", dict(E=30)), ("alias", dict(alias=True))]
REP_CASES, FLAG_CASES = {}, {}


def rep_case(family, id, part, **kw):
    """a case of the family's representative; ns is the unforced one of the base shape unless given"""
    _key, hid, name, pieces, P, waves, fb, opt = _BY_KEY[REPS[family]]
    kw.setdefault("ns", 1 if name == P32 else 4)
    return case(id, part, family, hid, name, pieces, P, waves=waves, fallback=fb, **kw, **opt)


for _fam in REPS:
    REP_CASES[_fam] = rep_case(_fam, f"rep-{_fam}", 2)
    for _flag, _kw in FLAGS:
        if _flag == "alias":
            if not REP_CASES[_fam]["fallback"]:
                continue                # (F aliasing x under the default mode: the families of the fp16 build)
            _c = rep_case(_fam, f"rep-{_fam}-alias", 2, alias=True)
            _c["name"], _c["fallback"] = _c["name"].replace("cc_fwd_f16<", "cc_fwd_bf16<"), 0
        else:
            _c = rep_case(_fam, f"rep-{_fam}-{_flag}", 2, **_kw)
        FLAG_CASES[_fam, _flag] = _c

# ---- part 3: tile and node edges ------------------------------------------------------------------------------------------------------
# (family, net, options, {P: (name, pieces, waves, fallback)}): P = 1 and fwd_p = 2; the 32-wide kernel has P = 2 only
_g8p2 = f16("T=8,PARTS=2,P=2,EXACT=0,LIVE=0")
EDGE_REPS = [
    ("f16-exact13/pipe", N50, {}, {1: (f16("T=4,PARTS=2,P=1,EXACT=1,LIVE=13"), 2, 4, 1), 2: (f16("T=4,PARTS=2,P=2,EXACT=1,LIVE=13,PIPE"), 2, 4, 1)}),
    ("f16-wide-first", [100, 50, 50], {}, {1: (f16("T1=7,TREST=4,PARTS=2,P=1,EXACT=1,LIVE=13"), 2, 4, 1), 2: (_g8p2, 2, 4, 1)}),
    ("f16-t7-w8", [100] * 3, {}, {1: (f16("T=7,PARTS=2,P=1,EXACT=1,LIVE=26,WAVES=8"), 2, 8, 1), 2: (_g8p2, 2, 4, 1)}),
    ("bf16-3", N50, PREC["bf16x6"], {1: (bf16("T=4,PARTS=3,P=1,EXACT=1,LIVE=13"), 3, 4, 0), 2: (bf16("T=4,PARTS=3,P=2,EXACT=1,LIVE=13"), 3, 4, 0)}),
    ("p32", N50, dict(fwd_pipe=2, **PREC["bf16x3"]), {2: (P32, 2, 4, 0)}),
    ("fp32-tail", N50, PREC["fp32"], {1: ("cc_fwd<T=4,KS=13,P=1,TAIL=1>", 0, 4, 0), 2: ("cc_fwd<T=4,KS=13,P=2,TAIL=1>", 0, 4, 0)}),
]
COUNT_SHAPES = [(1, 1), (15, 1), (16, 1), (17, 1), (31, 1), (32, 1), (33, 1), (63, 1), (64, 1), (65, 1), (127, 1), (43, 3)]      # B d = .., 129
COUNT_CASES = []
for _fam, _hid, _opt, _byP in EDGE_REPS:
    for _P, (_name, _pieces, _waves, _fb) in _byP.items():
        for _B, _d in COUNT_SHAPES:
            for _ns in (1, None):       # whole, and split by the rule: at most 9 tiles, n = 20 -> 4 (the 32-wide kernel never splits)
                COUNT_CASES.append(case(f"count-{_fam}-p{_P}-{_B}x{_d}-ns{_ns or 'auto'}", 3, _fam, _hid, _name, _pieces, _P,
                                        1 if (_ns or _name == P32) else 4, _waves, _fb, B=_B, d=_d,
                                        **(dict(fwd_p=2) if _P == 2 else {}), **(dict(fwd_ns=1) if _ns else {}), **_opt))
NODE_N, NODE_NS = [1, 2, 3, 6, 7, 33], [1, 2, 4]
NODE_CASES = []
# Every representative at P = 1 and at fwd_p = 2.  The pipelined loop is the one whose node loop differs (layer 1 of a tile's next
# node, and that node's abscissa and weight, are formed one node ahead, from k_lo, the index clamped at n): it also runs at LIVE=0
# and in the bf16 build, so a part of a single node (2 nodes over 2 parts), ranges of 2 and 3 nodes and 7 nodes over 4 parts meet
# its prologue and its clamp in every form.
NODE_REPS = EDGE_REPS + [
    ("f16-pipe-live0", N60, {}, {2: (f16("T=4,PARTS=2,P=2,EXACT=1,LIVE=0,PIPE"), 2, 4, 1)}),
    ("bf16-pipe-live13", N50, PREC["bf16x3"], {2: (bf16("T=4,PARTS=2,P=2,EXACT=1,LIVE=13,PIPE"), 2, 4, 0)}),
    ("bf16-pipe-live0", N60, PREC["bf16x3"], {2: (bf16("T=4,PARTS=2,P=2,EXACT=1,LIVE=0,PIPE"), 2, 4, 0)}),
]
for _fam, _hid, _opt, _byP in NODE_REPS:
    for _P, (_name, _pieces, _waves, _fb) in _byP.items():
        for _n in NODE_N:
            for _ns in NODE_NS:         # more parts than nodes: the plan runs the range whole (7 nodes over 4 parts and 2 over 2 stay split)
                _want = 1 if (_name == P32 or _ns > _n + 1) else _ns
                NODE_CASES.append(case(f"nodes-{_fam}-p{_P}-n{_n}-ns{_ns}", 3, _fam, _hid, _name, _pieces, _P, _want, _waves, _fb, n=_n,
                                       fwd_ns=_ns, **(dict(fwd_p=2) if _P == 2 else {}), **_opt))
# pipelined against plain at fwd_p = 2: (net, LIVE) x build x (whole, split)
PIPE_PAIRS = []
for _hid, _live in ((N50, 13), (N60, 0), (PADDED, 0)):
    for _pre, _stem, _fb, _prec in (("f16", f16, 1, {}), ("bf16", bf16, 0, PREC["bf16x3"])):
        for _ns in (1, 4):
            _kw = dict(P=2, ns=_ns, fallback=_fb, fwd_p=2, **(dict(fwd_ns=1) if _ns == 1 else {}), **_prec)
            _body = f"T=4,PARTS=2,P=2,EXACT=1,LIVE={_live}"
            PIPE_PAIRS.append((case(f"pipe=1-{_pre}-{tag(_hid)}-ns{_ns}", 3, "pipe-vs-plain", _hid, _stem(_body + ",PIPE"), fwd_pipe=1, **_kw),
                               case(f"pipe=0-{_pre}-{tag(_hid)}-ns{_ns}", 3, "pipe-vs-plain", _hid, _stem(_body), fwd_pipe=0, **_kw)))
        if _hid is PADDED:
            continue
        for _n in NODE_N:               # ... and over the short and unevenly split node ranges of NODE_CASES
            for _ns in NODE_NS:
                _kw = dict(P=2, ns=1 if _ns > _n + 1 else _ns, fallback=_fb, n=_n, fwd_p=2, fwd_ns=_ns, **_prec)
                PIPE_PAIRS.append((case(f"pipe=1-{_pre}-{tag(_hid)}-n{_n}-ns{_ns}", 3, "pipe-vs-plain", _hid, _stem(_body + ",PIPE"), fwd_pipe=1, **_kw),
                                   case(f"pipe=0-{_pre}-{tag(_hid)}-n{_n}-ns{_ns}", 3, "pipe-vs-plain", _hid, _stem(_body), fwd_pipe=0, **_kw)))

# ---- part 4: the flow entries on the part 2 representatives ---------------------------------------------------------------------------
FLOW_CASES = {}
for _fam in REPS:
    FLOW_CASES[_fam] = {"fp32": rep_case(_fam, f"flow-{_fam}", 4, x0=False),
                        "x-bf16": rep_case(_fam, f"flow-{_fam}-x-bf16", 4, x0=False, x_bf16=True),
                        "h-bf16": rep_case(_fam, f"flow-{_fam}-h-bf16", 4, x0=False, h_bf16=True),
                        "xh-bf16": rep_case(_fam, f"flow-{_fam}-xh-bf16", 4, x0=False, x_bf16=True, h_bf16=True)}
LL_SHAPES = [(37, 1), (37, 3), (9, 17), (5, 63)]      # rows start and end inside tiles and inside P = 2 pairs: 37, 111, 153, 315 integrals
LL_CASES = []
for _fam in REPS:
    for _B, _d in LL_SHAPES:
        for _ns in (1, None):           # at most 20 tiles: the rule splits four ways
            LL_CASES.append(rep_case(_fam, f"ll-{_fam}-{_B}x{_d}-ns{_ns or 'auto'}", 4, x0=False, B=_B, d=_d,
                                     **(dict(ns=1, fwd_ns=1) if _ns else {})))
# z_2 saved: every T1 x LIVE of the wide-first family; three hidden layers (the three-stage backward holds 2..4 after the cut)
Z2_CASES = [case(f"z2-t{_t1}-live{_live}", 4, "f16-wide-first", [_w1] + _rest, f16(f"T1={_t1},TREST=4,PARTS=2,P=1,EXACT=1,LIVE={_live}"),
                 fallback=1, x0=False) for _t1, _w1 in WIDE_FIRST_W1.items() for _live, _rest in ((13, [50, 50]), (0, [60, 60]))]

BY_ID = {c["id"]: c for c in CASES}


def plan_flags(c):
    return ((_lib.PLAN_MARKER_ALIASED if c["alias"] else 0) | (_lib.PLAN_X_BF16 if c["x_bf16"] else 0) | (_lib.PLAN_H_BF16 if c["h_bf16"] else 0))


def mlp_desc(c):
    m = desc(c)
    m.hidden_act, m.out_act = c["act"], c["out_act"]
    return m


# ---- inputs -----------------------------------------------------------------------------------------------------------------------
def make_net(c):
    """IntegrandNetwork of the case on the CPU, default-initialised from a seed of its own, parameters x 1.7."""
    import umnn_amd
    with torch.random.fork_rng(devices=[]):
        torch.manual_seed(2000 + 7 * sum(c["hid"]) + 31 * len(c["hid"]) + c["E"])
        net = umnn_amd.IntegrandNetwork(c["d"], 1 + c["E"], list(c["hid"]), 1, act_func="Sigmoid" if c["out_act"] == SIGMOID else "ELU")
    if c["act"] == RELU:
        for i in range(1, 2 * len(c["hid"]), 2):
            net.net[i] = torch.nn.ReLU()
    with torch.no_grad():
        for p in net.parameters():
            p.mul_(1.7)
    return net


def _input_key(c):
    return (tuple(c["hid"]), c["act"], c["out_act"], c["B"], c["d"], c["E"], c["x_bf16"], c["h_bf16"])


_INPUTS, _REFERENCE = {}, {}


def inputs(c):
    """-> namespace(net, x, x0, h, scaling, lj_in: float32 CPU tensors holding values of the storage type).  Computed once per distinct
    input set and shared by every case and test that asks for it; nothing in it is modified afterwards."""
    key = _input_key(c)
    if key not in _INPUTS:
        B, d, E = c["B"], c["d"], c["E"]
        gen = torch.Generator().manual_seed(4099 + 131 * B + 17 * d + E)
        xdt = torch.bfloat16 if c["x_bf16"] else torch.float32
        hdt = torch.bfloat16 if c["h_bf16"] else torch.float32
        draw = lambda shape, scale, dt: (torch.randn(*shape, generator=gen) * scale).to(dt).float()
        _INPUTS[key] = types.SimpleNamespace(net=make_net(c), x=draw((B, d), 2.0, xdt), x0=draw((B, d), 0.3, xdt), h=draw((B, E * d), 1.0, hdt),
                                             scaling=draw((d,), 0.1, torch.float32), lj_in=draw((B, d), 1.0, xdt))
    return _INPUTS[key]


def cc_tables_rounded(n, dtype=np.float32):
    """the float32-rounded Clenshaw-Curtis tables the kernels read (compute_cc_weights), widened to `dtype`"""
    return tuple(t.reshape(-1).numpy().astype(dtype) for t in compute_cc_weights(n))


def quadrature64(net, x0, x, h, n, inv_f=False):
    """(F, f(x), f(x0)) in float64 (torch) on float32-rounded weights, inputs and tables -- the truth.  x0 None: zeros."""
    net64 = copy.deepcopy(net).double()
    w, s = (torch.from_numpy(t) for t in cc_tables_rounded(n, np.float64))
    x, h = x.double(), h.double()
    x0 = torch.zeros_like(x) if x0 is None else x0.double()
    B, d = x.shape
    with torch.no_grad():
        xT = x0 + n * ((x - x0) / n)
        t = x0[:, None, :] + (xT - x0)[:, None, :] * (s[None, :, None] + 1) / 2
        hs = h[:, None, :].expand(B, n + 1, h.shape[1]).reshape(B * (n + 1), -1)
        f = net64(t.reshape(B * (n + 1), d), hs).view(B, n + 1, d)
        if inv_f:
            f = 1 / f
        F = (f * w[None, :, None]).sum(1) * (xT - x0) / 2
        return F.numpy(), net64(x, h).numpy(), net64(x0, h).numpy()


def oracle_net(net, dtype):
    lins = [m for m in net.net if isinstance(m, torch.nn.Linear)]
    relu = any(isinstance(m, torch.nn.ReLU) for m in net.net)
    sigmoid = isinstance(net.net[-1], torch.nn.Sigmoid)
    return O.Net([l.weight.detach().numpy().astype(dtype) for l in lins], [l.bias.detach().numpy().astype(dtype) for l in lins],
                 O.RELU if relu else O.LEAKY, O.SIGMOID if sigmoid else O.ELU1)


def reference(c, x=None):
    """-> namespace(F, fx, fx0: the float64 truth; e32: rel_err of the reference's float32 arithmetic (oracle.cc_oracle on float32
    arrays) against it, per output; E32: max(e32, 2^-22)).  Computed once per distinct (input set, n, x0, inv_f) and cached; `x`
    replaces the case's x (the second block of a chain) and is not cached."""
    key = _input_key(c) + (c["n"], c["x0"], c["inv_f"])
    if x is None and key in _REFERENCE:
        return _REFERENCE[key]
    i = inputs(c)
    xx = i.x if x is None else x
    x0 = i.x0 if c["x0"] else None
    F, fx, fx0 = quadrature64(i.net, x0, xx, i.h, c["n"], c["inv_f"])
    n32 = oracle_net(i.net, np.float32)
    a, a0, ah = xx.numpy(), (i.x0.numpy() if c["x0"] else np.zeros_like(xx.numpy())), i.h.numpy()
    F32 = O.integrate_parallel(n32, a0, a, ah, c["n"], inv_f=c["inv_f"])
    assert F32.dtype == np.float32
    e32 = (U.rel_err(F32, F), U.rel_err(O.integrand(n32, a, ah), fx), U.rel_err(O.integrand(n32, a0, ah), fx0))
    out = types.SimpleNamespace(F=F, fx=fx, fx0=fx0, e32=e32, E32=tuple(max(e, FLOOR) for e in e32))
    if x is None:
        _REFERENCE[key] = out
    return out


def bounds(c):
    """(bound of F, of f(x), of f(x0)) as rel_err figures: M x E32, never above the outer 1e-4"""
    return tuple(min(M(c) * e, OUTER) for e in reference(c).E32)


# ---- derived quantities of the flow entries ---------------------------------------------------------------------------------------
def flow_reference(c, x=None, lj_in=False):
    """Float64 z and log_jac of a block (lower limit 0) with their per-element ABSOLUTE bounds, from the truth and the bounds above.
      log_jac = log(f + 1e-10) + s: an error df of f moves it by df / f; |df| <= bound(f_x) max(f, 1), and max(f, 1) / f = 1 / min(f, 1).
          The fp32 log, the add of s (and of log_jac_in) round to 2^-22 max(1, |lj|) in all.
      z = exp(s) (F + h_0): an error dF of F moves it by exp(s) dF, |dF| <= bound(F) max(|F|, 1).  The add, the product and v_exp_f32
          (one ulp; the exponent's own rounding is |s| 2^-24) are three roundings of operands no larger than exp(s) (|F| + |h_0|):
          2^-22 of that, or of 1 where it is smaller."""
    i, r = inputs(c), reference(c, x)
    bF, bfx, _ = (min(M(c) * e, OUTER) for e in r.E32)
    s, d = i.scaling.double().numpy()[None, :], c["d"]
    h0 = i.h.double().numpy()[:, :d]
    lj = np.log(r.fx + 1e-10) + s + (i.lj_in.double().numpy() if lj_in else 0.0)
    z = np.exp(s) * (r.F + h0)
    blj = bfx / np.minimum(r.fx, 1.0) + FLOOR * np.maximum(1.0, np.abs(lj))
    bz = np.exp(s) * bF * np.maximum(np.abs(r.F), 1.0) + FLOOR * np.maximum(1.0, np.exp(s) * (np.abs(r.F) + np.abs(h0)))
    return types.SimpleNamespace(z=z, lj=lj, bz=bz, blj=blj, ref=r)


LOG_2PI = float(np.log(2 * np.pi))


def chain_x2(c):
    """the input of block 2 of the two-block chain: the truth of block 1's z, reversed, rounded to fp32 (so the chain's truth does not
    depend on the device)"""
    return torch.from_numpy(np.ascontiguousarray(flow_reference(c).z[:, ::-1]).astype(np.float32))


def ll_reference(c):
    """Two blocks (the case's net, h and scaling twice; block 2 reads chain_x2): ll = sum_i lj_1 + sum_i lj_2 - 1/2 sum_i (log 2 pi +
    z_2^2) in float64, and its per-row absolute bound: the sum over the row of the per-element bounds -- an error dz of z_2 moves
    z_2^2 / 2 by |z_2| dz + dz^2 / 2 -- plus d x 2^-24 x sum |terms| for the fp32 row sums (d - 1 additions per block and the
    accumulation of block 2 onto block 1)."""
    r1, r2 = flow_reference(c), flow_reference(c, chain_x2(c))
    g = 0.5 * (LOG_2PI + r2.z ** 2)
    ll = (r1.lj + r2.lj - g).sum(1)
    terms = (np.abs(r1.lj) + np.abs(r2.lj) + g).sum(1)
    bll = (r1.blj + r2.blj + np.abs(r2.z) * r2.bz + 0.5 * r2.bz ** 2).sum(1) + c["d"] * 2.0 ** -24 * terms
    return types.SimpleNamespace(ll=ll, bll=bll, r1=r1, r2=r2)
