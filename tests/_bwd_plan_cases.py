"""The case table of the backward launch plan (csrc/cc_bwd_plan.h): which kernel a backward call runs, by net, shape, flags and
options.  Shared by tests/test_backward_plan_cpu.py (umnn_cc_backward_plan_name, no GPU), tests/test_gpu_backward_plan.py (the same
query against what a call really notes) and tools/path_identity.py (bit-identity of two checkouts).

The expected names were derived by hand from the launchers as they stood BEFORE the plan header existed (plan_backward_impl /
backward_impl in cc_backward.hip, umnn_launch_backward_bf16, umnn_launch_backward_front), for a device of 256 CUs (MI355X; also what
the library assumes without a device):
  * tiles = ceil(B d / 16); a tile's nodes are split (ns > 1) when 2 tiles <= 4 x 256 waves; the grid is min(256, ceil(tiles ns / 4));
  * bf16x3: every hidden layer of <= 4 tiles, at least one of >= 3, 2..4 hidden layers: the bf16 families.  Four hidden layers,
    bwd_ws, ns == 1 and tiles >= 4 x grid: the workgroup pipeline -- on fp16 pieces when bwd_ws16 == 2 or (== 1 and B d (n + 1) >=
    2^21), the output is ELU+1, the call does not integrate 1/f and n + 1 <= 256; else bwd_swp: the pipelined loop; else the
    round-2 loop.  LIVE=13 when every hidden layer is 48..51 wide, else LIVE=0;
  * first hidden layer of 5..8 tiles over 2..4 layers of <= 4: three stages; the middle stage is the pipeline (FRONT,WS) when four
    layers follow the cut, bwd_ws and the chunk has >= 4 x grid tiles; on fp16 pieces under the rule above for a single chunk;
    bwd_precision fp32: the six-term build (cc_bwd_bf16x6<...>), one-pass middle stage;
  * everything else: the fp32 passes; unequal widths above four tiles are zero-padded to the (5, 17), (7, 26) or (8, 32) family that
    holds them, and the call notes its LAST pass (EDGE=0 when the edge pass does not hold every layer's dW)."""
from umnn_amd import _lib

ELU, SIGMOID = _lib.OUT_ELU_PLUS_ONE, _lib.OUT_SIGMOID
N50 = [50] * 4
FRONT = [100, 50, 50, 50, 50]
FP32 = _lib.PRECISIONS["fp32"]
INV_F, G_FX = 1, 2      # UMNN_PLAN_INV_F, UMNN_PLAN_G_FX (literal: tools/path_identity.py also runs this file in checkouts without the query)


def case(id, hid, B, d, n, name, E=30, flags=0, out_act=ELU, gpu=False, **options):
    return dict(id=id, hid=list(hid), B=B, d=d, n=n, name=name, E=E, flags=flags, out_act=out_act, gpu=gpu, options=options)


def _boundary(E, gpu):
    # B d = 16384: 1024 tiles = 4 x 256 workgroups, and 16384 x 128 nodes = 2^21 evaluations -- on both boundaries at once
    return [
        case(f"boundary-f16-E{E}", N50, 1024, 16, 127, "cc_bwd_f16<L=4,LIVE=13,WS>", E=E, gpu=gpu),
        case(f"boundary-n126-E{E}", N50, 1024, 16, 126, "cc_bwd_bf16<L=4,LIVE=13,WS>", E=E, gpu=gpu),
        case(f"boundary-B1023-E{E}", N50, 1023, 16, 127, "cc_bwd_bf16<L=4,LIVE=13,SWP>", E=E, gpu=gpu),
    ]


CASES = _boundary(30, False) + _boundary(6, True) + [
    # bwd_ws16 = 2: "whenever eligible" -- what is not eligible keeps the bf16 pipeline
    case("ws16=2-n256", N50, 300, 63, 256, "cc_bwd_bf16<L=4,LIVE=13,WS>", bwd_ws16=2),          # 257 nodes > W16_MAX_NODES
    case("ws16=2-n255", N50, 300, 63, 255, "cc_bwd_f16<L=4,LIVE=13,WS>", bwd_ws16=2),
    case("ws16=2-inv_f", N50, 300, 63, 20, "cc_bwd_bf16<L=4,LIVE=13,WS>", flags=INV_F, bwd_ws16=2),
    case("ws16=2-sigmoid", N50, 300, 63, 20, "cc_bwd_bf16<L=4,LIVE=13,WS>", out_act=SIGMOID, bwd_ws16=2),
    case("ws16=2-n256-small", N50, 1024, 16, 256, "cc_bwd_bf16<L=4,LIVE=13,WS>", E=6, gpu=True, bwd_ws16=2),
    case("ws16=2-inv_f-small", N50, 1024, 16, 20, "cc_bwd_bf16<L=4,LIVE=13,WS>", E=6, flags=INV_F, gpu=True, bwd_ws16=2),
    case("ws16=2-sigmoid-small", N50, 1024, 16, 20, "cc_bwd_bf16<L=4,LIVE=13,WS>", E=6, out_act=SIGMOID, gpu=True, bwd_ws16=2),
    # the options one by one, each on top of the one before: 300 x 63 x 121 nodes is above 2^21, so the default would be fp16 pieces
    case("default-300x63", N50, 300, 63, 120, "cc_bwd_f16<L=4,LIVE=13,WS>"),
    case("ws16=0", N50, 300, 63, 120, "cc_bwd_bf16<L=4,LIVE=13,WS>", bwd_ws16=0),
    case("ws=0", N50, 300, 63, 120, "cc_bwd_bf16<L=4,LIVE=13,SWP>", bwd_ws16=0, bwd_ws=0),
    case("swp=0", N50, 300, 63, 120, "cc_bwd_bf16<L=4,EDGE=1,LIVE=13>", bwd_ws16=0, bwd_ws=0, bwd_swp=0),
    case("ws16=0-small", N50, 1024, 16, 127, "cc_bwd_bf16<L=4,LIVE=13,WS>", E=6, gpu=True, bwd_ws16=0),
    case("ws=0-small", N50, 1024, 16, 127, "cc_bwd_bf16<L=4,LIVE=13,SWP>", E=6, gpu=True, bwd_ws16=0, bwd_ws=0),
    case("swp=0-small", N50, 1024, 16, 127, "cc_bwd_bf16<L=4,EDGE=1,LIVE=13>", E=6, gpu=True, bwd_ws16=0, bwd_ws=0, bwd_swp=0),
    # shapes that are not on the pipeline
    case("three-hidden", [50] * 3, 300, 63, 20, "cc_bwd_bf16<L=3,LIVE=13,SWP>"),
    case("small-batch", N50, 64, 63, 20, "cc_bwd_bf16<L=4,LIVE=13,SWP>"),                      # 252 tiles: node range split in four
    case("mixed-widths", [48, 60, 36, 50], 300, 63, 20, "cc_bwd_bf16<L=4,LIVE=0,WS>"),
    case("mixed-widths-small", [48, 60, 36, 50], 1024, 16, 20, "cc_bwd_bf16<L=4,LIVE=0,WS>", E=6, gpu=True),
    case("two-tiles", [20, 20], 9, 3, 12, "cc_bwd<T=2,NACC=3,EDGE=1,KS=0>", E=4, gpu=True),
    case("fp32-50x4", N50, 300, 63, 20, "cc_bwd<T=4,NACC=3,EDGE=1,KS=13>", bwd_precision=FP32),
    case("fp32-pad17", [66, 60], 9, 3, 12, "cc_bwd<T=5,NACC=2,EDGE=1,KS=17>", E=4, bwd_precision=FP32),
    case("fp32-pad26", [100, 80, 70], 9, 3, 12, "cc_bwd<T=7,NACC=1,EDGE=0,KS=26>", E=4, gpu=True, bwd_precision=FP32),
    case("fp32-pad26-two", [70, 90], 9, 3, 12, "cc_bwd<T=7,NACC=1,EDGE=1,KS=26>", E=4, bwd_precision=FP32),
    case("fp32-pad32", [120, 112, 116], 9, 3, 12, "cc_bwd<T=8,NACC=1,EDGE=0,KS=32>", E=4, bwd_precision=FP32),
    case("pad26-default", [100, 80, 70], 9, 3, 12, "cc_bwd<T=7,NACC=1,EDGE=0,KS=26>", E=4),        # (no bf16 family holds it either)
    # deep unequal wide nets: the padded images exceed the LDS; the net's own counts fit (generic kernels) or do not either ("")
    case("deep-wide-generic", [100, 80, 70, 90, 70], 9, 3, 12, "cc_bwd<T=7,NACC=1,EDGE=0,KS=0>", E=4),
    case("deep-wide-none", [120, 112, 116, 124], 9, 3, 12, "", E=4),
    # wide first hidden layer: three stages
    case("front", FRONT, 40, 784, 12, "cc_bwd_bf16<L=4,LIVE=13,WS,FRONT>"),
    case("front-ws=0", FRONT, 40, 784, 12, "cc_bwd_bf16<L=4,EDGE=1,LIVE=13,FRONT>", bwd_ws=0),
    case("front-ws16=2", FRONT, 40, 784, 12, "cc_bwd_f16<L=4,LIVE=13,WS,FRONT>", bwd_ws16=2),
    case("front-fp32", FRONT, 40, 784, 12, "cc_bwd_bf16x6<L=4,EDGE=1,LIVE=13,FRONT>", bwd_precision=FP32),
    case("front-small", FRONT, 40, 784, 12, "cc_bwd_bf16<L=4,LIVE=13,WS,FRONT>", E=6, gpu=True),
    case("front-ws=0-small", FRONT, 40, 784, 12, "cc_bwd_bf16<L=4,EDGE=1,LIVE=13,FRONT>", E=6, gpu=True, bwd_ws=0),
    case("front-ws16=2-small", FRONT, 40, 784, 12, "cc_bwd_f16<L=4,LIVE=13,WS,FRONT>", E=6, gpu=True, bwd_ws16=2),
    case("front-fp32-small", FRONT, 40, 784, 12, "cc_bwd_bf16x6<L=4,EDGE=1,LIVE=13,FRONT>", E=6, gpu=True, bwd_precision=FP32),
    case("front-g_fx", FRONT, 40, 784, 12, "cc_bwd_bf16<L=4,LIVE=13,WS,FRONT>", flags=G_FX),
    case("front-few-tiles", FRONT, 9, 3, 12, "cc_bwd_bf16<L=4,EDGE=1,LIVE=13,FRONT>", E=4),         # 2 tiles: no pipeline
]
GPU_CASES = [c for c in CASES if c["gpu"]]


def desc(c, ptr=0x1000):
    """struct umnn_mlp of a case with placeholder pointers (the plan reads widths and activations only)"""
    widths = [1 + c["E"]] + c["hid"] + [1]
    m = _lib.MlpDesc()
    m.n_linear = len(widths) - 1
    for i, w in enumerate(widths):
        m.widths[i] = w
    for l in range(m.n_linear):
        m.W[l], m.b[l] = ptr, ptr
    m.hidden_act, m.out_act = _lib.ACT_LEAKY_RELU, c["out_act"]
    return m


def run(c, dev):
    """One backward call of the case on `dev`, fixed seeds, under the case's options -> (dx0, dx, dh, dtheta)."""
    import torch
    import umnn_amd
    from umnn_amd import integral as I
    from umnn_amd.nets import mlp_spec
    B, d, E = c["B"], c["d"], c["E"]
    torch.manual_seed(len(c["hid"]) + c["hid"][0])
    net = umnn_amd.IntegrandNetwork(d, 1 + E, c["hid"], 1, act_func="Sigmoid" if c["out_act"] == SIGMOID else "ELU").to(dev)
    gen = torch.Generator().manual_seed(B + d)
    x, h, g = (torch.randn(B, w, generator=gen).to(dev) for w in (d, E * d, d))
    with _lib.options(**c["options"]):
        return I.hip_backward(mlp_spec(net), None, x, h, g, None, c["n"], inv_f=bool(c["flags"] & INV_F))
