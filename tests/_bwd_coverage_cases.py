"""Case table, inputs, float64 truth, arithmetic classes and error yardsticks of the quadrature-backward coverage tests: tests/test_backward_coverage_cpu.py (names,
completeness, the kink guard and the truth pin, no GPU) and tests/test_gpu_backward_coverage.py (every case on the device).

Names.  Every expected name below was derived by hand from csrc/cc_bwd_plan.h for a device of 256 CUs, not read back from the
library:
  * tiles = ceil(B d / 16).  Unforced, a tile's nodes are split ns = min(32, 1024 / tiles) ways when 2 tiles <= 1024 waves; bwd_ns
    = k forces ns = k; the route clamps ns to n + 1.  grid = min(256, ceil(tiles ns / 4)).
  * bf16x3, 2..4 hidden layers of <= 4 tiles, one of >= 3 (a layer of width H has (H + 16) // 16 tiles): four hidden layers, bwd_ws,
    ns == 1 and tiles >= 4 grid -> the workgroup pipeline (WS; cc_bwd_f16 under bwd_ws16 = 2 unless inv_f / sigmoid / n + 1 > 256);
    else bwd_swp -> SWP; else the round-2 loop (EDGE=1).  LIVE=13 when every hidden layer is 48..51 wide, else 0.  At 8 tiles
    bwd_ns = 1 gives grid 2 and 8 >= 4 x 2; at 9 tiles grid 3 and 9 < 12.
  * first hidden layer of 5..8 tiles (T1) over 2..4 layers of <= 4 tiles: three stages (FRONT).  L and LIVE are those of the layers
    after the cut; the stage kernels' NL2 is 13 when (width_2 + 4) // 4 == 13, else 0.  Unforced at 8 tiles the grid cap is 64, so the
    middle stage is the one-pass loop; bwd_ns = 1 makes it 2 and four layers after the cut run the pipeline (WS,FRONT).
    bwd_precision = fp32: the three-piece build, cc_bwd_bf16x6<..,FRONT>, one-pass middle stage always.  Stage C: front_bwd2 = 0 one
    wave per tile (bwd), 1 two waves per tile (bwd2; on fp16 pieces, bwd16, behind the fp16 middle stage), 2 bwd2 always.
  * everything else: fp32 passes, cc_bwd<T,NACC,EDGE,KS>.  The EDGE=1 pass holds best_nacc(T, 1, KS) layers of dW, every further
    pass (EDGE=0) best_nacc(T, 0, KS); the call notes its LAST pass.  `also` lists the first pass of a two-pass case where that
    kernel can never be a last pass (NACC=0: it holds no dW layer, so another pass always follows).

Inputs.  At these sizes one hidden pre-activation on the other side of zero moves d_theta by ~1 / (node evaluations) of its largest
entry (cc_bwd_plan.h: 4e-5 at 4e5 evaluations, i.e. 2e-2 at 861), far above any tolerance, and the truth is discontinuous there.
So rows are drawn by rejection, in float64 on the CPU from a fixed seed, rounded to the storage type (fp32 or bf16) first: a row is
kept only when the smallest |z| / (sum_k |W_jk a_k| + |b_j|) over every hidden unit of every hidden layer, at all n + 1 nodes and at
x and x0, of each of its d integrals, is at least GUARD = 1e-5 -- thirty times the 3e-7 relative noise cc_bwd_plan.h documents for the
fp16-piece recompute, a hundred times the fp32 figure.  At most half of the drawn rows of any case may be rejected (asserted on the
CPU).  The net is IntegrandNetwork default-initialised with its parameters x 1.7 (tests/test_gpu_round3.py)."""
import types

import numpy as np
import torch

from tests import _truth64
from umnn_amd import _lib
from umnn_amd.quadrature import compute_cc_weights

ELU, SIGMOID = _lib.OUT_ELU_PLUS_ONE, _lib.OUT_SIGMOID
LEAKY, RELU = _lib.ACT_LEAKY_RELU, _lib.ACT_RELU
FP32 = _lib.PRECISIONS["fp32"]
GUARD = 1e-5
LOW_GUARD = 3e-6        # the cases of 256 to 258 nodes only (the fp16 node-table limit, the chunked scratch): ten times the 3e-7 noise figure
REJECT_CAP = 0.5

CASES = []


def case(id, part, family, hid, name, B=41, d=3, E=4, n=6, act=LEAKY, out_act=ELU, x0=True, g_fx=True, inv_f=False, x_bf16=False,
         h_bf16=False, launches=None, guard=GUARD, also=(), **options):
    c = dict(id=id, part=part, family=family, hid=list(hid), name=name, B=B, d=d, E=E, n=n, act=act, out_act=out_act, x0=x0, g_fx=g_fx,
             inv_f=inv_f, x_bf16=x_bf16, h_bf16=h_bf16, launches=launches, guard=guard, also=tuple(also), options=options)
    assert all(o["id"] != id for o in CASES), id
    CASES.append(c)
    return c


def tag(hid):
    return "x".join(map(str, hid))


# ---- part 1: every variant by name; B = 41, d = 3: 123 integrals in 8 tiles, the last of 11 lanes -------------------------------
def _onepass(hid, live, ks):
    t = tag(hid)
    case(f"ws-{t}", 1, "WS", hid, f"cc_bwd_bf16<L=4,LIVE={live},WS>", bwd_ns=1)
    case(f"swp-{t}", 1, "SWP", hid, f"cc_bwd_bf16<L=4,LIVE={live},SWP>", bwd_ns=1, bwd_ws=0)
    case(f"loop-{t}", 1, "LOOP", hid, f"cc_bwd_bf16<L=4,EDGE=1,LIVE={live}>", bwd_ns=1, bwd_ws=0, bwd_swp=0)
    case(f"ws16-{t}", 1, "WS16", hid, f"cc_bwd_f16<L=4,LIVE={live},WS>", bwd_ns=1, bwd_ws16=2)
    case(f"fp32-{t}", 1, "FP32", hid, f"cc_bwd<T=4,NACC=3,EDGE=1,KS={ks}>", bwd_ns=1, bwd_precision=FP32)


_onepass([50] * 4, 13, 13)
_onepass([48, 60, 36, 50], 0, 0)
_onepass([60] * 4, 0, 0)                # (a first hidden layer above 56 units: registers 14 and 15 of the LIVE=0 kernels hold features too)
for _hid, _L, _live in (([50] * 3, 3, 13), ([50] * 2, 2, 13), ([40, 56, 33], 3, 0), ([60, 60], 2, 0)):
    case(f"swp-{tag(_hid)}", 1, "SWP", _hid, f"cc_bwd_bf16<L={_L},LIVE={_live},SWP>", bwd_ns=1)
    case(f"loop-{tag(_hid)}", 1, "LOOP", _hid, f"cc_bwd_bf16<L={_L},EDGE=1,LIVE={_live}>", bwd_ns=1, bwd_swp=0)
case("swp-9-tiles", 1, "SWP", [50] * 4, "cc_bwd_bf16<L=4,LIVE=13,SWP>", B=47, bwd_ns=1)        # 9 tiles < 4 x 3 workgroups

# three stages: T1 = 5, 6, 7, 8 over every (L, LIVE) after the cut
FRONT_W1 = {70: 5, 90: 6, 100: 7, 120: 8}
FRONT_RESTS = [([50, 50], 2, 13, 13), ([60, 60], 2, 0, 0), ([50, 50, 50], 3, 13, 13), ([48, 60, 36], 3, 0, 13), ([50] * 4, 4, 13, 13),
               ([60] * 4, 4, 0, 0)]                                  # (rest, L, LIVE, NL2 of the stage kernels)
for _w1 in FRONT_W1:
    for _rest, _L, _live, _nl2 in FRONT_RESTS:
        _hid = [_w1] + _rest
        case(f"front-{tag(_hid)}", 1, "FRONT", _hid, f"cc_bwd_bf16<L={_L},EDGE=1,LIVE={_live},FRONT>")
        case(f"front-p3-{tag(_hid)}", 1, "FRONT_P3", _hid, f"cc_bwd_bf16x6<L={_L},EDGE=1,LIVE={_live},FRONT>", bwd_precision=FP32)
        if _L == 4:
            case(f"front-ws-{tag(_hid)}", 1, "FRONT_WS", _hid, f"cc_bwd_bf16<L=4,LIVE={_live},WS,FRONT>", bwd_ns=1)
            case(f"front-ws16-{tag(_hid)}", 1, "FRONT_WS16", _hid, f"cc_bwd_f16<L=4,LIVE={_live},WS,FRONT>", bwd_ns=1, bwd_ws16=2)

# the fp32 variants; B = 9, d = 3: two tiles, the second of 11 lanes.  launches: main passes + d_h + the d_theta reduction
_F = dict(B=9, bwd_precision=FP32)
case("fp32-20x20", 1, "FP32", [20, 20], "cc_bwd<T=2,NACC=3,EDGE=1,KS=0>", **_F)
case("fp32-20x5", 1, "FP32_2", [20] * 5, "cc_bwd<T=2,NACC=3,EDGE=0,KS=0>", launches=4, **_F)
case("fp32-50x5", 1, "FP32_2", [50] * 5, "cc_bwd<T=4,NACC=3,EDGE=0,KS=13>", launches=4, **_F)
case("fp32-40x3", 1, "FP32", [40] * 3, "cc_bwd<T=4,NACC=3,EDGE=1,KS=0>", **_F)
case("fp32-40x5", 1, "FP32_2", [40] * 5, "cc_bwd<T=4,NACC=3,EDGE=0,KS=0>", launches=4, **_F)
case("fp32-64x2", 1, "FP32", [64, 64], "cc_bwd<T=5,NACC=2,EDGE=1,KS=17>", **_F)
case("fp32-64x4", 1, "FP32_2", [64] * 4, "cc_bwd<T=5,NACC=3,EDGE=0,KS=17>", launches=4, **_F)
case("fp32-100x2", 1, "FP32", [100, 100], "cc_bwd<T=7,NACC=1,EDGE=1,KS=26>", **_F)
case("fp32-100x3", 1, "FP32_2", [100] * 3, "cc_bwd<T=7,NACC=1,EDGE=0,KS=26>", **_F)
case("fp32-124x2", 1, "FP32_2", [124] * 2, "cc_bwd<T=8,NACC=1,EDGE=0,KS=32>", also=["cc_bwd<T=8,NACC=0,EDGE=1,KS=32>"], **_F)
case("fp32-pad32", 1, "PAD", [120, 112, 116], "cc_bwd<T=8,NACC=1,EDGE=0,KS=32>", also=["cc_bwd<T=8,NACC=0,EDGE=1,KS=32>"], **_F)
# deep unequal wide nets whose zero-padded images exceed the LDS: the generic kernels on the net's own counts
case("fp32-generic7", 1, "GENERIC", [100, 80, 70, 90, 70], "cc_bwd<T=7,NACC=1,EDGE=0,KS=0>", also=["cc_bwd<T=7,NACC=0,EDGE=1,KS=0>"], **_F)
case("fp32-generic8", 1, "GENERIC", [120, 20, 20, 20, 20, 20], "cc_bwd<T=8,NACC=1,EDGE=0,KS=0>", also=["cc_bwd<T=8,NACC=0,EDGE=1,KS=0>"], **_F)
NO_KERNEL = [[120, 112, 116, 124], [100] * 5]                      # (neither the padded nor the own images fit: the call is an error)

# ---- part 2: the flags on one representative per family ---------------------------------------------------------------------------
# (family, net, name, name when the fp16 pipeline is not eligible, launches, options)
REPS = [
    ("LOOP", [50] * 4, "cc_bwd_bf16<L=4,EDGE=1,LIVE=13>", None, 3, dict(bwd_ns=1, bwd_ws=0, bwd_swp=0)),
    ("SWP", [50] * 4, "cc_bwd_bf16<L=4,LIVE=13,SWP>", None, 3, dict(bwd_ns=1, bwd_ws=0)),
    ("WS", [50] * 4, "cc_bwd_bf16<L=4,LIVE=13,WS>", None, 3, dict(bwd_ns=1)),
    ("WS16", [50] * 4, "cc_bwd_f16<L=4,LIVE=13,WS>", "cc_bwd_bf16<L=4,LIVE=13,WS>", 3, dict(bwd_ns=1, bwd_ws16=2)),
    ("FRONT", [100, 50, 50, 50], "cc_bwd_bf16<L=3,EDGE=1,LIVE=13,FRONT>", None, 3, dict()),
    ("FRONT_WS", [100] + [50] * 4, "cc_bwd_bf16<L=4,LIVE=13,WS,FRONT>", None, 3, dict(bwd_ns=1)),
    ("FRONT_WS16", [100] + [50] * 4, "cc_bwd_f16<L=4,LIVE=13,WS,FRONT>", "cc_bwd_bf16<L=4,LIVE=13,WS,FRONT>", 3, dict(bwd_ns=1, bwd_ws16=2)),
    ("FRONT_P3", [100, 50, 50, 50], "cc_bwd_bf16x6<L=3,EDGE=1,LIVE=13,FRONT>", None, 3, dict(bwd_precision=FP32)),
    ("FP32", [50] * 4, "cc_bwd<T=4,NACC=3,EDGE=1,KS=13>", None, 3, dict(bwd_precision=FP32)),
    ("FP32_2", [50] * 5, "cc_bwd<T=4,NACC=3,EDGE=0,KS=13>", None, 4, dict(bwd_precision=FP32)),
    ("PAD", [100, 80, 70], "cc_bwd<T=7,NACC=1,EDGE=0,KS=26>", None, 4, dict(bwd_precision=FP32)),
]
FLAGS = [("no-x0", dict(x0=False)), ("no-g_fx", dict(g_fx=False)), ("inv_f", dict(inv_f=True)), ("sigmoid", dict(out_act=SIGMOID)),
         ("relu", dict(act=RELU)), ("x-bf16", dict(x_bf16=True)), ("h-bf16", dict(h_bf16=True)), ("xh-bf16", dict(x_bf16=True, h_bf16=True))]
REP_CASES = {}
for _fam, _hid, _name, _name_bf16, _launches, _opt in REPS:
    REP_CASES[_fam] = case(f"rep-{_fam}", 2, _fam, _hid, _name, launches=_launches, **_opt)
    for _flag, _kw in FLAGS:
        _ineligible = _name_bf16 is not None and (_kw.get("inv_f") or _kw.get("out_act") == SIGMOID)
        case(f"rep-{_fam}-{_flag}", 2, _fam, _hid, _name_bf16 if _ineligible else _name, launches=_launches, **_kw, **_opt)
# the fp16 pipeline's node tables hold 256 nodes: n = 255 runs it, n = 256 keeps the bf16 pipeline.  (Above n = 33 no draw meets the
# rejection cap at GUARD; these two are named and run, finite and reproducible, and held to the truth at LOW_GUARD with d = 1.)
case("ws16-n255", 2, "WS16", [50] * 4, "cc_bwd_f16<L=4,LIVE=13,WS>", B=123, d=1, n=255, guard=LOW_GUARD, bwd_ns=1, bwd_ws16=2)
case("ws16-n256", 2, "WS16", [50] * 4, "cc_bwd_bf16<L=4,LIVE=13,WS>", B=123, d=1, n=256, guard=LOW_GUARD, bwd_ns=1, bwd_ws16=2)
case("ws16-n1", 2, "WS16", [50] * 4, "cc_bwd_f16<L=4,LIVE=13,WS>", n=1, bwd_ns=1, bwd_ws16=2)
NEED_MASKS = [(0, 1, 1, 1), (1, 0, 1, 1), (1, 1, 0, 1), (1, 1, 1, 0), (1, 0, 0, 0), (0, 1, 0, 0), (0, 0, 1, 0), (0, 0, 0, 1)]

# ---- part 3: the node-range split; B = 9, d = 3: two tiles, the second of 11 lanes ------------------------------------------------
# unforced: ns = min(32, 1024 waves / 2 tiles) = 32; the route clamps to n + 1.  (The padded family is the two-layer 70-90 net, zero-padded to
# (7, 26): the 250 hidden units of 100-80-70 do not meet the rejection cap at n = 33.)
SPLIT_FAMILIES = [
    ("LOOP", [50] * 4, "cc_bwd_bf16<L=4,EDGE=1,LIVE=13>", 3, dict(bwd_ws=0, bwd_swp=0)),
    ("SWP4", [50] * 4, "cc_bwd_bf16<L=4,LIVE=13,SWP>", 3, dict(bwd_ws=0)),
    ("SWP3", [50] * 3, "cc_bwd_bf16<L=3,LIVE=13,SWP>", 3, dict()),
    ("SWP2", [60, 60], "cc_bwd_bf16<L=2,LIVE=0,SWP>", 3, dict()),
    ("FP32", [50] * 4, "cc_bwd<T=4,NACC=3,EDGE=1,KS=13>", 3, dict(bwd_precision=FP32)),
    ("FP32_2", [50] * 5, "cc_bwd<T=4,NACC=3,EDGE=0,KS=13>", 4, dict(bwd_precision=FP32)),
    ("PAD", [70, 90], "cc_bwd<T=7,NACC=1,EDGE=1,KS=26>", 3, dict(bwd_precision=FP32)),
]
SPLIT_NS = [1, 2, 3, 7, 32, None]
SPLIT_N = [1, 6, 32, 33]
SPLIT_CASES = {}
for _fam, _hid, _name, _launches, _opt in SPLIT_FAMILIES:
    for _n in SPLIT_N:
        SPLIT_CASES[_fam, _n] = [case(f"split-{_fam}-n{_n}-ns{'auto' if _ns is None else _ns}", 3, _fam, _hid, _name, B=9, n=_n,
                                      launches=_launches, **({} if _ns is None else dict(bwd_ns=_ns)), **_opt) for _ns in SPLIT_NS]

# ---- part 4: three-stage specifics ------------------------------------------------------------------------------------------------
# stage C: every (T1, NL2) with one wave per tile (front_bwd2 = 0), and bf16 stage C behind the fp16 middle stage (front_bwd2 = 2);
# front_bwd2 = 1 is the default of part 1 (bwd2 behind the bf16 middle stages, bwd16 behind the fp16 one)
STAGE_C = {}
for _w1 in FRONT_W1:
    for _rest, _live in (([50, 50], 13), ([60, 60], 0)):
        _hid = [_w1] + _rest
        for _b2 in (0, 2):
            STAGE_C["FRONT", _w1, _live, _b2] = case(f"front-bwd2={_b2}-{tag(_hid)}", 4, "FRONT", _hid, f"cc_bwd_bf16<L=2,EDGE=1,LIVE={_live},FRONT>", front_bwd2=_b2)
    for _rest, _live in (([50] * 4, 13), ([60] * 4, 0)):
        _hid = [_w1] + _rest
        for _b2 in (0, 2):
            STAGE_C["FRONT_WS", _w1, _live, _b2] = case(f"front-ws-bwd2={_b2}-{tag(_hid)}", 4, "FRONT_WS", _hid, f"cc_bwd_bf16<L=4,LIVE={_live},WS,FRONT>", bwd_ns=1, front_bwd2=_b2)
            STAGE_C["FRONT_WS16", _w1, _live, _b2] = case(f"front-ws16-bwd2={_b2}-{tag(_hid)}", 4, "FRONT_WS16", _hid, f"cc_bwd_f16<L=4,LIVE={_live},WS,FRONT>", bwd_ns=1, bwd_ws16=2,
                                                          front_bwd2=_b2)
# z_2 saved by the training forward (umnn_cc_backward_saved: lower limit 0, no d_x0), every T1 x NL2, with and without g_fx
Z2_CASES = {}
for _w1 in FRONT_W1:
    for _rest, _live in (([50, 50], 13), ([60, 60], 0)):
        for _gfx in (True, False):
            Z2_CASES[_w1, _live, _gfx] = case(f"front-z2-{tag([_w1] + _rest)}-{'g_fx' if _gfx else 'no-g_fx'}", 4, "FRONT", [_w1] + _rest,
                                             f"cc_bwd_bf16<L=2,EDGE=1,LIVE={_live},FRONT>", x0=False, g_fx=_gfx)
# the same pair with a bf16 embedding (the MNIST-shaped training path): T1 = 5 and 8, NL2 = 13 and 0, with g_fx, run through the C
# entries umnn_flow_stack_block_forward_save_io / umnn_cc_backward_saved_io with an io descriptor.  (A four-part key: the tests that walk
# the three-part keys above go through the Python wrappers.)
for _w1 in (70, 120):
    for _rest, _live in (([50, 50], 13), ([60, 60], 0)):
        Z2_CASES[_w1, _live, True, "h-bf16"] = case(f"front-z2-{tag([_w1] + _rest)}-g_fx-h-bf16", 4, "FRONT", [_w1] + _rest,
                                                    f"cc_bwd_bf16<L=2,EDGE=1,LIVE={_live},FRONT>", x0=False, g_fx=True, h_bf16=True)
# Several chunks.  The scratch holds (2 x 257 + 1) slices per tile (sized for n = 256 with g_fx); a call needs 2 (n + 1) + 1 with g_fx, so
# n = 257 (517 > 515) is the smallest n that does not fit: chunk = 8 x 515 // 517 = 7 of 8 tiles, evened out to two chunks of four.
# d = 1, B = 123: 8 tiles of rows.  The launch counter counts one per main pass whatever the chunks (umnn_bwd_launch notes once), so
# the delta stays 3: the chunking shows in the byte pattern behind the exactly-sized workspace, whose last region is this scratch.
# 258 nodes do not fit the fp16 pipeline's tables and a chunk of 4 tiles is below 4 x 2 workgroups: bwd_ws16 = 2 keeps bf16, one-pass.
case("front-chunks", 4, "FRONT", [70, 50, 50], "cc_bwd_bf16<L=2,EDGE=1,LIVE=13,FRONT>", B=123, d=1, n=257, guard=LOW_GUARD, launches=3)
case("front-chunks-ws16=2", 4, "FRONT", [70] + [50] * 4, "cc_bwd_bf16<L=4,EDGE=1,LIVE=13,FRONT>", B=123, d=1, n=257, guard=LOW_GUARD, launches=3,
     bwd_ns=1, bwd_ws16=2)
case("front-one-chunk", 4, "FRONT", [70, 50, 50], "cc_bwd_bf16<L=2,EDGE=1,LIVE=13,FRONT>", B=123, d=1, n=256, guard=LOW_GUARD, launches=3)

# ---- part 5: the finishing kernels; the 20-20 net with n = 2, so the main pass is negligible ---------------------------------------
# d_h: the matrix-core kernel takes E <= 80 and ceil(B d / 16) >= 8 x 256 tiles, i.e. B d >= 32768 - 15.  d = 16 divides 32768 - 16 and
# 32768; 32768 - 15 = 7 x 4679 is run with d = 7.
DH = {}
for _B, _d in ((2047, 16), (4679, 7), (2048, 16)):
    for _E in (1, 15, 16, 17, 80, 81):
        _mfma = _B * _d >= 32768 - 15 and _E <= 80
        DH[_B * _d, _E] = (case(f"dh-{_B * _d}-E{_E}", 5, "FINISH", [20, 20], "cc_bwd<T=2,NACC=3,EDGE=1,KS=0>", B=_B, d=_d, E=_E, n=2),
                           "cc_bwd_dh<mfma>" if _mfma else "cc_bwd_dh")
DH[32768, "50x4"] = (case("dh-32768-50x4", 5, "FINISH", [50] * 4, "cc_bwd_bf16<L=4,LIVE=13,WS>", B=2048, d=16, n=2), "cc_bwd_dh<mfma>")
# dW1[:, 1:]: ceil(H1 / 16) x ceil((E + 1) / 16) output tiles over four waves: 2 x 1 -> <2>, 7 x 2 -> <4>, 7 x 6 = 42 -> <10> in two launches
case("dw0-20-E4", 5, "FINISH", [20, 20], "cc_bwd<T=2,NACC=3,EDGE=1,KS=0>", n=2)
case("dw0-100-E30", 5, "FINISH", [100, 100], "cc_bwd<T=7,NACC=1,EDGE=1,KS=26>", E=30, n=2)
case("dw0-100-E90", 5, "FINISH", [100, 100], "cc_bwd<T=7,NACC=1,EDGE=1,KS=26>", E=90, n=2)
# dW1 chunk (bwd_plan_shape): 64 integrals, halved while B d / chunk < 2 x 256: 64 from B d = 32768 (above), 32 from 16384, else 16 (B d = 123)
case("dw0-chunk32", 5, "FINISH", [20, 20], "cc_bwd<T=2,NACC=3,EDGE=1,KS=0>", B=1025, d=16, n=2)       # 16400 integrals, a last chunk of 16
case("dw0-chunk32-exact", 5, "FINISH", [20, 20], "cc_bwd<T=2,NACC=3,EDGE=1,KS=0>", B=1024, d=16, n=2)

BY_ID = {c["id"]: c for c in CASES}


def plan_flags(c):
    return ((_lib.PLAN_INV_F if c["inv_f"] else 0) | (_lib.PLAN_G_FX if c["g_fx"] else 0) | (_lib.PLAN_X_BF16 if c["x_bf16"] else 0)
            | (_lib.PLAN_H_BF16 if c["h_bf16"] else 0))


def desc(c, ptr=0x1000):
    """struct umnn_mlp of a case with placeholder pointers (the plan reads widths and activations only)"""
    widths = [1 + c["E"]] + c["hid"] + [1]
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
        torch.manual_seed(1000 + 7 * sum(c["hid"]) + 31 * len(c["hid"]) + c["E"])
        net = umnn_amd.IntegrandNetwork(c["d"], 1 + c["E"], list(c["hid"]), 1, act_func="Sigmoid" if c["out_act"] == SIGMOID else "ELU")
    if c["act"] == RELU:
        for i in range(1, 2 * len(c["hid"]), 2):
            net.net[i] = torch.nn.ReLU()
    with torch.no_grad():
        for p in net.parameters():
            p.mul_(1.7)
    return net


def margin_rows(net, x0, x, h, n, chunk=256):
    """[R]: per row, the smallest |z| / (sum_k |W_jk a_k| + |b_j|) over every hidden unit of every hidden layer at the n + 1 nodes
    t_k = x0 + (x - x0)(s_k + 1) / 2 and at x and x0 themselves, of each of the row's d integrals; numpy float64."""
    lins = [m for m in net.net if isinstance(m, torch.nn.Linear)]
    Ws = [l.weight.detach().double().numpy() for l in lins[:-1]]
    bs = [l.bias.detach().double().numpy() for l in lins[:-1]]
    relu = any(isinstance(m, torch.nn.ReLU) for m in net.net)
    s = compute_cc_weights(n)[1].double().numpy().reshape(-1)            # (the float32-rounded nodes the kernels and the truth read)
    R, d = x.shape
    E = h.shape[1] // d
    out = np.empty(R)
    for lo in range(0, R, chunk):
        xa, x0a, ha = x[lo:lo + chunk], x0[lo:lo + chunk], h[lo:lo + chunk]
        r = xa.shape[0]
        t = np.concatenate([x0a[:, None, :] + (xa - x0a)[:, None, :] * (s[None, :, None] + 1) / 2, xa[:, None, :], x0a[:, None, :]], 1)
        K = t.shape[1]
        hb = np.broadcast_to(ha.reshape(r, 1, E, d).transpose(0, 1, 3, 2), (r, K, d, E))        # h is feature-major: index e d + i
        a = np.concatenate([t[..., None], hb], -1).reshape(r * K * d, 1 + E)
        m = np.full(r, np.inf)
        for W, b in zip(Ws, bs):
            z = a @ W.T + b
            mag = np.abs(a) @ np.abs(W).T + np.abs(b)
            m = np.minimum(m, (np.abs(z) / np.maximum(mag, 1e-300)).reshape(r, -1).min(1))
            a = np.maximum(z, 0) if relu else np.where(z > 0, z, 0.01 * z)
        out[lo:lo + chunk] = m
    return out


def _input_key(c):
    return (tuple(c["hid"]), c["act"], c["out_act"], c["B"], c["d"], c["E"], c["n"], c["x0"], c["g_fx"], c["x_bf16"], c["h_bf16"], c["guard"])


_INPUTS, _TRUTH = {}, {}


def inputs(c):
    """-> namespace(net, x0, x, h, g, g_fx: float64 CPU tensors holding values of the storage type, None where the case passes none;
    reject: the fraction of drawn rows rejected; margin: the smallest margin of a kept row).  Computed once per distinct input set
    and shared by every case and test that asks for it; nothing in it is modified afterwards."""
    key = _input_key(c)
    if key in _INPUTS:
        return _INPUTS[key]
    net = make_net(c)
    B, d, E, n = c["B"], c["d"], c["E"], c["n"]
    gen = torch.Generator().manual_seed(7919 + 131 * B + 17 * d + E + 1009 * n)
    xdt = torch.bfloat16 if c["x_bf16"] else torch.float32
    hdt = torch.bfloat16 if c["h_bf16"] else torch.float32
    kept, margins, drawn, used = [], [], 0, 0
    while used < B:                                   # rows are examined in the order drawn, block by block, up to the B-th kept one
        R = 2 * B + 32
        blk = [(torch.randn(R, w, generator=gen, dtype=torch.float64) * sc).to(dt).double()
               for w, sc, dt in ((d, 2.0, xdt), (d, 0.3, xdt), (E * d, 1.0, hdt), (d, 1.0, xdt), (d, 1.0, xdt))]
        x, x0, h = blk[0], (blk[1] if c["x0"] else torch.zeros_like(blk[1])), blk[2]
        m = margin_rows(net, x0.numpy(), x.numpy(), h.numpy(), n)
        ok = np.flatnonzero(m >= c["guard"])[:B - used]
        drawn += R if used + len(ok) < B else int(ok[-1]) + 1
        used += len(ok)
        kept.append([t[ok] for t in blk])
        margins.append(m[ok])
    x, x0, h, g, gfx = (torch.cat([k[i] for k in kept]) for i in range(5))
    out = types.SimpleNamespace(net=net, x=x, x0=x0 if c["x0"] else None, h=h, g=g, g_fx=gfx if c["g_fx"] else None,
                                reject=1.0 - B / drawn, margin=float(np.concatenate(margins).min()))
    _INPUTS[key] = out
    return out


def truth(c, device="cpu", dtype=torch.float64):
    """tests/_truth64.backward_reference on the case's inputs and the float32-rounded weights the kernels read -> (d_x0, d_x, d_h,
    d_theta) in `dtype` on `device` (float64: the truth; float32: the reference's own arithmetic).  Computed once and shared."""
    key = _input_key(c) + (c["inv_f"], str(device), dtype)
    if key not in _TRUTH:
        i = inputs(c)
        to = lambda t: None if t is None else t.to(device)
        _TRUTH[key] = tuple(t.detach() for t in _truth64.backward_reference(i.net, to(i.x0), to(i.x), to(i.h), to(i.g), to(i.g_fx), c["n"],
                                                                            dtype=dtype, chunk=1024, inv_f=c["inv_f"]))
    return _TRUTH[key]


# ---- arithmetic classes and yardsticks ----------------------------------------------------------------------------------------------
# What the kernel headers declare, not what was measured:
#   A (fp32 level): d_x0 and d_x of every family -- the Leibniz terms and the g_fx tangent come from the forward recompute, which is
#     fp32 (cc_backward.hip) or three pieces / six cross terms "fp32-level accuracy" (cc_bwd_bf16_kernel.h) everywhere --; every output
#     of cc_bwd<...> (fp32), cc_bwd_f16<...> (two fp16 pieces of 11 bits, cc_bwd_ws16_kernel.h) and cc_bwd_bf16x6<...> (UMNN_BWD_NPB = 3:
#     six cross terms in the delta chain and the dW products too).
#   B (two bf16 pieces, three cross terms, "errors stay ~1e-5": cc_bwd_bf16_kernel.h): d_h and d_theta of cc_bwd_bf16<...> in all its
#     forms (loop, SWP, WS, FRONT, WS+FRONT; also where a flag made the fp16 pipeline ineligible, so that the expected name is the
#     bf16 one), and of the fp16 middle stage with a bf16 stage C behind it.  cc_bwd_plan.h: stage C is BWD16 (fp16 pieces) only when
#     front_bwd2 == 1; front_bwd2 = 2 (BWD2) and front_bwd2 = 0 (BWD, one wave per tile) both run the two-piece bf16 build of
#     cc_backward_front.hip behind the fp16 middle stage.
OUTPUTS = ("d_x0", "d_x", "d_h", "d_theta")
M_GRAD = 8.0          # the project's constant: M_GRAD of tests/_multi_coverage_cases.py, M_FP32_LEVEL of tests/_fwd_coverage_cases.py
# output -> M where the measured ratio asks for more than M_GRAD: twice the largest measured ratio (profiles/bwd_coverage/README.md).  Never
# d_x / d_x0.
#   "d_theta:b_out", the gradient of the output bias, a parameter tensor of ONE element: the single sum of dout = cot f'(s) over all
#   B d (n + 1) points (+ the g_fx term), whose terms change sign -- sum |dout| / |sum dout| is 13 .. 16000 over the input sets here.  Its
#   fp32 rounding error is a few units of 2^-24 times that cancellation, in the kernels (the fma chain `dwo`, the lane shuffles, the
#   partial sums of the reduction kernel) as in ATen; but where a tensor of many elements takes the largest of many such errors, E32 of
#   this one is ONE draw, anywhere between 0.00 and 0.96 of cancellation x 2^-24 over the input sets, often at the 2^-22 floor.  The five
#   runs that measure above 8 x E32 (8.1 .. 17.0: rep-FRONT_WS16-no-x0, rep-FRONT_WS-inv_f, rep-FRONT_WS16-inv_f, front-chunks-ws16=2,
#   front-z2-120x60x60-g_fx saved) all measure 0.35 .. 0.92 of cancellation x 2^-24: one fp32 rounding of that sum.  No product is involved.
M_OF = {"d_theta:b_out": 2 * 17.02}
FLOOR = 2.0 ** -22
TOL = 1e-4            # tests/test_gpu_backward.py (restated: that module needs a GPU to import)


def bf16_stage_c_behind_fp16(c):
    return c["name"].startswith("cc_bwd_f16<") and "FRONT" in c["name"] and c["options"].get("front_bwd2", 1) != 1


def arith_class(c):
    """-> {output: "A" | "B"} from the case's expected name and options (the rule above)."""
    two_piece = c["name"].startswith("cc_bwd_bf16<") or bf16_stage_c_behind_fp16(c)
    assert two_piece or c["name"].startswith(("cc_bwd<", "cc_bwd_f16<", "cc_bwd_bf16x6<")), c["name"]
    return {"d_x0": "A", "d_x": "A", "d_h": "B" if two_piece else "A", "d_theta": "B" if two_piece else "A"}


def split_layers(c):
    """Indices (into the net's Linear layers) of the layers whose backward products W_l^T delta and delta (x) a run on two bf16 pieces.
    cc_bwd_bf16<...>: every hidden-to-hidden layer -- in the three-stage forms the first of them is stage C's, the rest the middle
    stage's.  The fp16 middle stage with a bf16 stage C: that first one only.  The input layer is not among them (d_h and dW1 come from
    dc = sum_k delta_1 in the fp32 finishing kernels, dW1[:, 0] from an fp32 fma), nor is the output layer: every bf16 kernel forms
    delta_L = dout w_out act'(a_L) and dw_out += dout a_L in fp32 registers (`dwo`, `wout` in cc_bwd_bf16_kernel.h, cc_bwd_swp_kernel.h
    and cc_bwd_ws_kernel.h -- which is why the SWP and loop kernels agree bit for bit in the output layer)."""
    n_linear = len(c["hid"]) + 1
    if c["name"].startswith("cc_bwd_bf16<"):
        return tuple(range(1, n_linear - 1))
    return (1,) if bf16_stage_c_behind_fp16(c) else ()


def _pieces(t):
    """hi = bf16(t), lo = bf16(t - hi), both round to nearest even (of the float32 value the kernel holds), as float64"""
    hi = t.float().to(torch.bfloat16).to(t.dtype)
    return hi, (t - hi).float().to(torch.bfloat16).to(t.dtype)


class _TwoPieceLinear(torch.autograd.Function):
    """y = a W^T + b exactly; backward with every product on two bf16 pieces and the cross terms hi hi + hi lo + lo hi (the constant-one
    feature of the bias column is its own leading piece, so the bias gradient sums hi(delta) + lo(delta))."""

    @staticmethod
    def forward(ctx, a, W, b):
        ctx.save_for_backward(a, W)
        return torch.nn.functional.linear(a, W, b)

    @staticmethod
    def backward(ctx, g):
        a, W = ctx.saved_tensors
        (gh, gl), (ah, al), (Wh, Wl) = _pieces(g), _pieces(a), _pieces(W)
        return gh @ Wh + gh @ Wl + gl @ Wh, gh.t() @ ah + gh.t() @ al + gl.t() @ ah, (gh + gl).sum(0)


class _SplitLinear(torch.nn.Linear):
    def forward(self, a):
        return _TwoPieceLinear.apply(a, self.weight, self.bias)


def three_term_net(c):
    """A deep copy of the case's net whose split_layers(c) differentiate on two bf16 pieces; the forward stays exact."""
    import copy
    net = copy.deepcopy(inputs(c).net)
    lins = [m for m in net.net if isinstance(m, torch.nn.Linear)]
    for l in split_layers(c):
        lins[l].__class__ = _SplitLinear
    return net


def param_sizes(c):
    widths = [1 + c["E"]] + c["hid"] + [1]
    return [k for i in range(len(widths) - 1) for k in (widths[i] * widths[i + 1], widths[i + 1])]


def errors(c, outs, ref):
    """-> {output: error} of (d_x0, d_x, d_h, d_theta) `outs` against `ref` (torch tensors, None where absent): U.rel_err for d_x0 and
    d_x, U.scaled_err for d_h, the flat d_theta and -- under "tensors" -- each parameter tensor of d_theta separately."""
    from tests import _util as U
    np64 = lambda t: t.detach().double().cpu().numpy()
    crit = (U.rel_err, U.rel_err, U.scaled_err, U.scaled_err)
    e = {nm: None if o is None else crit[k](np64(o), np64(ref[k])) for k, (nm, o) in enumerate(zip(OUTPUTS, outs))}
    if outs[3] is not None:
        e["tensors"] = [U.scaled_err(a, b) for a, b in zip(np.split(np64(outs[3]), np.cumsum(param_sizes(c))[:-1]),
                                                           np.split(np64(ref[3]), np.cumsum(param_sizes(c))[:-1]))]
    return e


_YARD = {}


def yardsticks(c):
    """-> {output: yardstick, "tensors": [per parameter tensor]}, on the CPU, once per input set and class: E32 = the error of the
    reference's own float32 run against the float64 truth, floored at 2^-22; for class B outputs max(E32, E3), E3 the error of the
    float64 truth with the products of split_layers(c) on two bf16 pieces."""
    cls = arith_class(c)
    key = _input_key(c) + (c["inv_f"], split_layers(c))
    if key not in _YARD:
        ref = truth(c)
        floor = lambda e: {k: ([max(x, FLOOR) for x in v] if isinstance(v, list) else max(v, FLOOR)) for k, v in e.items()}
        y = floor(errors(c, truth(c, dtype=torch.float32), ref))
        if split_layers(c):
            i = inputs(c)
            e3 = floor(errors(c, [t.detach() for t in _truth64.backward_reference(three_term_net(c), i.x0, i.x, i.h, i.g, i.g_fx, c["n"],
                                                                                   chunk=1024, inv_f=c["inv_f"])], ref))
            y["E3"] = e3
            for nm in ("d_h", "d_theta"):
                y[nm] = max(y[nm], e3[nm])
            y["tensors"] = [max(a, b) for a, b in zip(y["tensors"], e3["tensors"])]
        _YARD[key] = y
    assert all(cls[nm] == ("B" if split_layers(c) and nm in ("d_h", "d_theta") else "A") for nm in OUTPUTS)
    return _YARD[key]


def bound_of(name):
    """M of one output: M_GRAD, or the entry of M_OF ("d_theta:b_out": the last parameter tensor)"""
    return M_OF.get(name, M_GRAD)


def check_bounds(c, outs, ref, tag=None):
    """Every output present in `outs` within M x its yardstick of `ref`, d_theta flat and per parameter tensor; prints the largest
    error / yardstick ratio per output, of the parameter tensors but the output bias, and of the output bias (BWDYARD lines), and
    -> those ratios."""
    y, e = yardsticks(c), errors(c, outs, ref)
    ratio = {nm: None if e[nm] is None else e[nm] / y[nm] for nm in OUTPUTS}
    per_tensor = [a / b for a, b in zip(e.get("tensors") or [], y["tensors"])]
    if per_tensor:
        ratio["tensors"], ratio["b_out"] = max(per_tensor[:-1]), per_tensor[-1]
    cls = arith_class(c)
    fmt = "|".join("-" if ratio.get(nm) is None else f"{ratio[nm]:.2f}" for nm in OUTPUTS + ("tensors", "b_out"))
    print(f"BWDYARD|{c['part']}|{c['family']}|{tag or c['id']}|{''.join(cls[nm] for nm in OUTPUTS)}|{fmt}")
    for nm in OUTPUTS:
        assert ratio[nm] is None or ratio[nm] <= bound_of(nm), (c["id"], nm, cls[nm], e[nm], y[nm], ratio[nm])
    for k, r in enumerate(per_tensor):
        name = "d_theta:b_out" if k == len(per_tensor) - 1 else f"d_theta:{'bW'[k % 2 == 0]}_{k // 2}"
        assert r <= bound_of(name), (c["id"], name, cls["d_theta"], e["tensors"][k], y["tensors"][k], r)
    return ratio
