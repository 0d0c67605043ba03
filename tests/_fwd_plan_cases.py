"""The case table of the launch plan of the forward quadrature, the bracket search and the Newton solve (csrc/cc_fwd_plan.h): which
kernel a call runs and with which P, node-range split (ns), waves per workgroup, grid and LDS bytes, by net, shape, flags and options.
Shared by tests/test_forward_plan_cpu.py (umnn_cc_launch_plan, no GPU), tests/test_gpu_forward_plan.py (the same query against what a
call really notes) and tools/path_identity.py (bit-identity of two checkouts).

The expectations were derived by hand from the launchers as they stood BEFORE the plan existed (launch_forward in cc_forward.hip,
umnn_launch_forward_bf16 / _f16 in cc_forward_bf16.hip, umnn_launch_forward_p32, inv_launch and inv_mode in cc_inv_launch.h), for a
device of 256 CUs (MI355X; also what the library assumes without a device) -- with one rule that is newer than those launchers: a
forced fwd_ns above n + 1 runs the node range whole, like an automatic one (the launchers took it as given, and part 0 of such a
split, whose wave publishes f(x), holds no node; tests/_fwd_coverage_cases.py has the cases):
  * forward: tiles = ceil(B d / 16); P = 2 from 8192 tiles (8 per SIMD); below 2048 tiles the node range is split, ns = 4 up to 1024
    tiles, else 2; fwd_p / fwd_ns override; ns > n + 1 -> 1, forced or not.  f16x3: the fp16 build (two pieces, bf16 build queued
    behind it) unless the marker output aliases an input (bf16 build, two pieces); bf16x3: two bf16 pieces; bf16x6: three.  What a
    build does not serve goes on to three bf16 pieces, then to fp32 MFMA; a single hidden layer and fwd_precision = fp32 are fp32 MFMA
    at once.
  * on a build: every hidden layer of the same 5..8 tiles (two pieces only): P = 1 unless fwd_p forces 2, ns = 4 up to 512 tiles, 2
    up to 1024; eight waves per workgroup when two workgroups of images (+ 1 KiB each) exceed 160 KiB.  First hidden layer of 5..8
    tiles over layers of <= 4 (two pieces, P = 1): the wide-first kernels, the same ns rule, LIVE=13 when layers 2..L are 48..51 wide.
    Else: tile bucket 2 / 4 / 8; EXACT when every layer fills the bucket; two pieces with fwd_pad: inexact nets of fwd_pad_min..4
    tiles are zero-padded to EXACT=1, T=4, LIVE=0.  EXACT, T=4, two pieces, fwd_pipe, nothing forced and >= 2048 tiles: P = 2, ns = 1;
    P = 2 there runs the PIPE variant however it came about.  fwd_pipe = 2 on the bf16 build with LIVE=13 and <= 5 hidden layers:
    the 32x32x16 kernel (32 integrals per wave).  LIVE = the common K-step count of four when a variant has it, else 0; no exact
    variant: the generic one (EXACT=0, LIVE=0).  Images: t_out x ceil(t_in / 2) x pieces KiB per layer pair (+ half steps for odd
    wide counts); split scratch: waves x 3 P x 16 floats.
  * fp32 MFMA: TAIL=1 when every hidden layer has the same width H with 16 (T - 1) <= H <= 16 (T - 1) + 3, fwd_tail allows it and the
    variant exists (only H - 16 (T - 1) = 2 does: widths 50); exact KS variants for (4, 13) and (7, 26), else generic T = 2 / 4 / 8.
  * search (one tile per sample) and solve (one tile per sixteen rows): f16x3, and fp32 / bf16x6 above four tiles: fp16 build; bf16x3:
    two bf16 pieces; fp32 / bf16x6 up to four tiles: three.  P = 1; 3..4-tile nets always padded; ns = waves per workgroup while
    tiles x waves <= 2048 and waves <= n + 1 (and, outside the wide-first family, the scratch of 16 / 32 floats per wave fits), else 1.
    (The generic T=4 rows of both tables cannot be reached: every 3..4-tile net is padded to the exact ones.)"""
from umnn_amd import _lib

FORWARD, SEARCH, SOLVE, SOLVE_BLOCK = 0, 1, 2, 3
Z2_SAVED, X_BF16, H_BF16, ALIASED = 4, 8, 16, 32      # UMNN_PLAN_* (literal: tools/path_identity.py also runs this file in checkouts without the query)
EUNSUPPORTED = -2
N50 = [50] * 4
N100 = [100] * 3
MNIST = [100, 50, 50, 50, 50]
P32 = "cc_fwd_bf16<32x32x16,PARTS=2,P=2,EXACT=1,LIVE=26,PIPE32>"


def case(id, hid, B, d, n, name, pieces=2, P=1, ns=1, waves=4, blocks=None, lds=None, fallback=1, kind=FORWARD, E=30, flags=0, rc=0,
         gpu=False, **options):
    return dict(id=id, hid=list(hid), B=B, d=d, n=n, name=name, pieces=pieces, P=P, ns=ns, waves=waves, blocks=blocks, lds=lds,
                fallback=fallback, kind=kind, E=E, flags=flags, rc=rc, gpu=gpu, options=options)


def f16(body):
    return f"cc_fwd_f16<{body}>"


def bf16(body):
    return f"cc_fwd_bf16<{body}>"


PREC = {k: dict(fwd_precision=v) for k, v in _lib.PRECISIONS.items()}
T4_13 = "T=4,PARTS=2,P=1,EXACT=1,LIVE=13"
PIPE = "T=4,PARTS=2,P=2,EXACT=1,LIVE=13,PIPE"
IMG50 = 3 * 4 * 2 * 2 * 1024      # [50]*4 on two pieces: three images of 4 tiles x 2 K-steps x 2 pieces of 1 KiB

FORWARD_CASES = [
    # the flagship shape and the batch-size rules around it
    case("c3", N50, 8192, 63, 100, f16(PIPE), P=2, blocks=4032, lds=IMG50),
    case("few-tiles", N50, 37, 3, 20, f16(T4_13), ns=4, blocks=7, lds=IMG50 + 768, gpu=True),
    case("pipe-2048-tiles", N50, 2048, 16, 4, f16(PIPE), P=2, blocks=256, lds=IMG50, gpu=True),
    case("pipe-2047-tiles", N50, 2047, 16, 4, f16(T4_13), ns=2, blocks=1024, lds=IMG50 + 768, gpu=True),
    case("few-nodes", N50, 37, 3, 2, f16(T4_13), blocks=2, lds=IMG50, gpu=True),                    # ns = 4 > n + 1
    case("bf16x6-few-tiles", N50, 37, 3, 20, bf16("T=4,PARTS=3,P=1,EXACT=1,LIVE=13"), pieces=3, ns=4, blocks=7, lds=IMG50 * 3 // 2 + 768,
         fallback=0, gpu=True, **PREC["bf16x6"]),
    case("bf16x6-8192-tiles", N50, 8192, 16, 4, bf16("T=4,PARTS=3,P=2,EXACT=1,LIVE=13"), pieces=3, P=2, blocks=1024, fallback=0, gpu=True,
         **PREC["bf16x6"]),
    case("bf16x6-8191-tiles", N50, 8191, 16, 4, bf16("T=4,PARTS=3,P=1,EXACT=1,LIVE=13"), pieces=3, blocks=2048, fallback=0, gpu=True,
         **PREC["bf16x6"]),
    case("bf16x3-few-tiles", N50, 37, 3, 20, bf16(T4_13), ns=4, blocks=7, lds=IMG50 + 768, fallback=0, gpu=True, **PREC["bf16x3"]),
    case("aliased", N50, 37, 3, 20, bf16(T4_13), ns=4, blocks=7, lds=IMG50 + 768, fallback=0, flags=ALIASED),
    # fp32 MFMA
    case("fp32-c3", N50, 8192, 63, 100, "cc_fwd<T=4,KS=13,P=2,TAIL=1>", pieces=0, P=2, blocks=4032, lds=(3 * 3 * 13 * 64 + 3 * 192) * 4,
         fallback=0, **PREC["fp32"]),
    case("fp32-few-tiles", N50, 37, 3, 20, "cc_fwd<T=4,KS=13,P=1,TAIL=1>", pieces=0, ns=4, blocks=7, fallback=0, gpu=True, **PREC["fp32"]),
    case("fp32-width-51", [51] * 4, 37, 3, 20, "cc_fwd<T=4,KS=13,P=1,TAIL=0>", pieces=0, ns=4, blocks=7, lds=3 * 4 * 13 * 64 * 4 + 768,
         fallback=0, gpu=True, **PREC["fp32"]),
    case("fp32-tail=0", N50, 37, 3, 20, "cc_fwd<T=4,KS=13,P=1,TAIL=0>", pieces=0, ns=4, blocks=7, fallback=0, gpu=True, fwd_tail=0,
         **PREC["fp32"]),
    case("one-hidden-layer", [50], 37, 3, 20, "cc_fwd<T=4,KS=13,P=1,TAIL=1>", pieces=0, ns=4, blocks=7, lds=768, fallback=0, gpu=True),
    case("fp32-width-100", N100, 37, 3, 20, "cc_fwd<T=7,KS=26,P=1,TAIL=0>", pieces=0, ns=4, blocks=7, fallback=0, **PREC["fp32"]),
    case("fp32-generic", [20, 20], 37, 3, 20, "cc_fwd<T=2,KS=0,P=1,TAIL=0>", pieces=0, ns=4, blocks=7, fallback=0, **PREC["fp32"]),
    # the 32x32x16 kernel: opt-in, bf16 build only
    case("pipe32", N50, 8192, 63, 100, P32, P=2, blocks=4032, lds=3 * 14 * 1024, fallback=0, fwd_pipe=2, **PREC["bf16x3"]),
    case("pipe32-few-tiles", N50, 37, 3, 20, P32, P=2, blocks=1, lds=3 * 14 * 1024, fallback=0, gpu=True, fwd_pipe=2, **PREC["bf16x3"]),
    case("pipe32-f16x3", N50, 8192, 63, 100, f16(PIPE), P=2, blocks=4032, fwd_pipe=2),
    case("pipe=0", N50, 2048, 16, 4, f16(T4_13), blocks=512, fwd_pipe=0),
    # uniform wide nets: P = 2 becomes P = 1 unless forced; one workgroup of images per CU -> eight waves
    case("wide-100", N100, 65536, 2, 20, f16("T=7,PARTS=2,P=1,EXACT=1,LIVE=26,WAVES=8"), waves=8, blocks=1024, lds=2 * 7 * 7 * 1024),
    case("wide-100-ns4", N100, 37, 3, 20, f16("T=7,PARTS=2,P=1,EXACT=1,LIVE=26,WAVES=8"), ns=4, waves=8, blocks=4,
         lds=2 * 7 * 7 * 1024 + 8 * 192, gpu=True),
    case("wide-100-ns2", N100, 600, 16, 20, f16("T=7,PARTS=2,P=1,EXACT=1,LIVE=26,WAVES=8"), ns=2, waves=8, blocks=150),
    case("wide-100-ns1", N100, 1025, 16, 20, f16("T=7,PARTS=2,P=1,EXACT=1,LIVE=26,WAVES=8"), waves=8, blocks=129),
    case("wide-100-two-layers", [100, 100], 37, 3, 20, f16("T=7,PARTS=2,P=1,EXACT=1,LIVE=26"), ns=4, blocks=7),     # one image: two workgroups per CU
    case("wide-100-p-forced", N100, 37, 3, 20, f16("T=8,PARTS=2,P=2,EXACT=0,LIVE=0"), P=2, ns=4, blocks=4, lds=2 * 7 * 4 * 2 * 1024 + 1536,
         fwd_p=2),
    # wide first hidden layer over a narrow rest
    case("wide-first", MNIST, 100, 784, 20, f16("T1=7,TREST=4,PARTS=2,P=1,EXACT=1,LIVE=13"), blocks=1225, lds=(14 + 3 * 8) * 2048),
    case("wide-first-few-tiles", MNIST, 37, 3, 20, f16("T1=7,TREST=4,PARTS=2,P=1,EXACT=1,LIVE=13"), ns=4, blocks=7, lds=(14 + 3 * 8) * 2048 + 768,
         gpu=True),
    case("wide-first-live-0", [100, 60, 60], 37, 3, 20, f16("T1=7,TREST=4,PARTS=2,P=1,EXACT=1,LIVE=0"), ns=4, blocks=7, lds=(14 + 8) * 2048 + 768,
         E=4, gpu=True),
    case("wide-first-z2", MNIST, 40, 784, 20, f16("T1=7,TREST=4,PARTS=2,P=1,EXACT=1,LIVE=13"), blocks=490, flags=Z2_SAVED),
    case("wide-first-z2-fp32", MNIST, 40, 784, 20, "", rc=EUNSUPPORTED, flags=Z2_SAVED, **PREC["fp32"]),
    case("z2-not-wide-first", N50, 40, 784, 20, "", rc=EUNSUPPORTED, flags=Z2_SAVED),
    case("wide-first-p-forced", MNIST, 37, 3, 20, f16("T=8,PARTS=2,P=2,EXACT=0,LIVE=0"), P=2, ns=4, blocks=4, fwd_p=2),
    # generic and padded
    case("two-tiles", [20, 20], 37, 3, 20, f16("T=2,PARTS=2,P=1,EXACT=0,LIVE=0"), ns=4, blocks=7, lds=4096 + 768, gpu=True),
    case("padded", [48, 60, 36, 50], 37, 3, 20, f16("T=4,PARTS=2,P=1,EXACT=1,LIVE=0"), ns=4, blocks=7, lds=IMG50 + 768, gpu=True),
    case("pad=0", [48, 60, 36, 50], 37, 3, 20, f16("T=4,PARTS=2,P=1,EXACT=0,LIVE=0"), ns=4, blocks=7, lds=(4 + 3 + 4) * 2 * 2 * 1024 + 768,
         gpu=True, fwd_pad=0),
    case("pad_min=4", [20, 40], 37, 3, 20, f16("T=4,PARTS=2,P=1,EXACT=0,LIVE=0"), ns=4, blocks=7, fwd_pad_min=4),     # three tiles at most
    case("padded-bf16x6", [48, 60, 36, 50], 37, 3, 20, bf16("T=4,PARTS=3,P=1,EXACT=0,LIVE=0"), pieces=3, ns=4, blocks=7, fallback=0,
         **PREC["bf16x6"]),                                                                                       # (only two pieces pad)
    case("mixed-wide", [70, 90], 37, 3, 20, f16("T=8,PARTS=2,P=1,EXACT=0,LIVE=0"), ns=4, blocks=7, E=4),
    case("mixed-wide-bf16x6", [70, 90], 37, 3, 20, "cc_fwd<T=8,KS=0,P=1,TAIL=0>", pieces=0, ns=4, blocks=7, fallback=0, E=4, **PREC["bf16x6"]),
    # forced P and ns
    case("p-forced", N50, 37, 3, 20, f16(PIPE), P=2, ns=4, blocks=4, lds=IMG50 + 1536, fwd_p=2),
    case("p-forced-1", N50, 8192, 63, 100, f16(T4_13), blocks=8064, fwd_p=1),
    case("ns-forced", N50, 2048, 16, 4, f16(T4_13), ns=2, blocks=1024, fwd_ns=2),
    # images above 160 KiB on every family
    case("images-exceed-lds", [120] * 7, 37, 3, 20, "", rc=EUNSUPPORTED, E=4),
]


def _inverse(kind, stem, rows):
    """search / solve cases of `rows` rows: tiles = rows (search) or ceil(rows / 16) (solve); scratch 16 / 32 floats per wave"""
    scratch = 64 if kind == SEARCH else 128      # bytes per wave
    tag = "search" if kind == SEARCH else "solve"

    def tiles(r):
        return r if kind == SEARCH else (r + 15) // 16

    def inv(id, hid, name, r=rows, waves=4, img=None, n=20, split=True, stem_=None, E=4, **kw):
        t, ns = tiles(r), (waves if split else 1)
        return case(f"{tag}-{id}", hid, r, 3, n, f"{stem_ or stem + '_f16'}<{name}>", ns=ns, waves=waves, blocks=-(-t // (waves // ns)),
                    lds=None if img is None else img + (scratch * waves if split else 0), kind=kind, E=E, **kw)

    bf = stem + "_bf16"
    KB = 1024
    return [
        # one case per row of the variant tables, small batch (ns = waves): exact, wide at four and at eight waves, generic
        inv("50x4", N50, "T=4,EXACT=1,LIVE=13", img=IMG50, gpu=True),
        inv("padded", [48, 60, 36, 50], "T=4,EXACT=1,LIVE=0", img=IMG50),
        inv("100x2", [100, 100], "T=7,EXACT=1,LIVE=26", img=7 * 7 * KB),
        inv("110x2", [110, 110], "T=7,EXACT=1,LIVE=0", img=7 * 7 * KB),
        inv("70x2", [70, 70], "T=5,EXACT=1,LIVE=0", img=5 * 5 * KB),
        inv("90x2", [90, 90], "T=6,EXACT=1,LIVE=0", img=6 * 6 * KB),
        inv("120x2", [120, 120], "T=8,EXACT=1,LIVE=0", img=8 * 8 * KB),
        inv("100x3", N100, "T=7,EXACT=1,LIVE=26,WAVES=8", waves=8, img=2 * 7 * 7 * KB, gpu=True),
        inv("110x3", [110] * 3, "T=7,EXACT=1,LIVE=0,WAVES=8", waves=8, img=2 * 7 * 7 * KB),
        inv("70x5", [70] * 5, "T=5,EXACT=1,LIVE=0,WAVES=8", waves=8, img=4 * 5 * 5 * KB),
        inv("90x4", [90] * 4, "T=6,EXACT=1,LIVE=0,WAVES=8", waves=8, img=3 * 6 * 6 * KB),
        inv("120x3", [120] * 3, "T=8,EXACT=1,LIVE=0,WAVES=8", waves=8, img=2 * 8 * 8 * KB),
        inv("two-tiles", [20, 20], "T=2,EXACT=0,LIVE=0", img=4 * KB),
        inv("mixed-wide", [70, 90], "T=8,EXACT=0,LIVE=0", img=6 * 3 * 2 * KB),
    ] + [inv(f"wide-first-{t1}-{live}", [w1] + rest, f"T1={t1},TREST=4,LIVE={live}", img=(4 * t1 + 16) * KB, gpu=(t1 == 7 and live == 13))
         for t1, w1 in ((5, 70), (6, 90), (7, 100), (8, 120)) for live, rest in ((13, [50, 50]), (0, [60, 60]))] + [
        # three pieces: fp32 / bf16x6 up to four tiles; above that the fp16 build; bf16x3: two bf16 pieces
        inv("bf16x6-50x4", N50, "T=4,PARTS=3,EXACT=1,LIVE=13", stem_=bf, pieces=3, fallback=0, img=IMG50 * 3 // 2, gpu=True, **PREC["bf16x6"]),
        inv("fp32-padded", [48, 60, 36, 50], "T=4,PARTS=3,EXACT=1,LIVE=0", stem_=bf, pieces=3, fallback=0, **PREC["fp32"]),
        inv("bf16x6-two-tiles", [20, 20], "T=2,PARTS=3,EXACT=0,LIVE=0", stem_=bf, pieces=3, fallback=0, **PREC["bf16x6"]),
        inv("fp32-100x3", N100, "T=7,EXACT=1,LIVE=26,WAVES=8", waves=8, **PREC["fp32"]),
        inv("bf16x3-100x3", N100, "T=7,EXACT=1,LIVE=26,WAVES=8", stem_=bf, waves=8, fallback=0, **PREC["bf16x3"]),
        inv("bf16x3-50x4", N50, "T=4,EXACT=1,LIVE=13", stem_=bf, fallback=0, gpu=True, **PREC["bf16x3"]),
        # the small-batch plan ends above tiles x waves = 8 x 256, and needs a node for every wave
        inv("512-tiles", N50, "T=4,EXACT=1,LIVE=13", r=512 if kind == SEARCH else 512 * 16, img=IMG50),
        inv("513-tiles", N50, "T=4,EXACT=1,LIVE=13", r=513 if kind == SEARCH else 512 * 16 + 1, img=IMG50, split=False),
        inv("256-tiles-8-waves", N100, "T=7,EXACT=1,LIVE=26,WAVES=8", r=256 if kind == SEARCH else 256 * 16, waves=8),
        inv("257-tiles-8-waves", N100, "T=7,EXACT=1,LIVE=26,WAVES=8", r=257 if kind == SEARCH else 256 * 16 + 1, waves=8, split=False),
        inv("few-nodes", N50, "T=4,EXACT=1,LIVE=13", n=2, img=IMG50, split=False, gpu=True),
        inv("few-nodes-8-waves", N100, "T=7,EXACT=1,LIVE=26,WAVES=8", waves=8, n=6, split=False),
        inv("dozens-of-rows", N50, "T=4,EXACT=1,LIVE=13", r=600 if kind == SEARCH else 600 * 16, img=IMG50, split=False, gpu=(kind == SEARCH)),
        # images of exactly 160 KiB: the scratch of a split does not fit, so the node range stays whole; one more tile: no kernel
        inv("scratch-does-not-fit", [120, 120, 100, 70], "T=8,EXACT=0,LIVE=0", img=160 * KB, split=False),
        case(f"{tag}-images-exceed-lds", [120] * 7, rows, 3, 20, "", rc=EUNSUPPORTED, kind=kind, E=4),
        case(f"{tag}-one-hidden-layer", [50], rows, 3, 20, "", rc=EUNSUPPORTED, kind=kind, E=4),
    ]


CASES = FORWARD_CASES + _inverse(SEARCH, "cc_invert", 10) + _inverse(SOLVE, "cc_solve", 37) + [
    # umnn_cc_solve_block: the rows are the B d flat index
    case("solve-block", N50, 37, 3, 20, "cc_solve_f16<T=4,EXACT=1,LIVE=13>", ns=4, blocks=7, lds=IMG50 + 512, kind=SOLVE_BLOCK, E=4, gpu=True),
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
    m.hidden_act, m.out_act = _lib.ACT_LEAKY_RELU, _lib.OUT_ELU_PLUS_ONE
    return m


def inputs(c):
    """(integrand network, x, h, scaling) of a case on the CPU, fixed seeds; x doubles as the target of the inverse jobs"""
    import torch
    import umnn_amd
    B, d, E = c["B"], c["d"], c["E"]
    torch.manual_seed(len(c["hid"]) + c["hid"][0])
    net = umnn_amd.IntegrandNetwork(d, 1 + E, c["hid"], 1)
    gen = torch.Generator().manual_seed(B + d)
    x, h = torch.randn(B, d, generator=gen), torch.randn(B, E * d, generator=gen)
    return net, x, h, torch.randn(d, generator=gen) * 0.1


SEARCH_ROUNDS = 8       # bracket one candidate step wide after k rounds: 100 / 9^k = 2.3e-6


def run(c, dev):
    """One call of the case on `dev` under the case's options -> tuple of output tensors.  forward: (F, f(x), f(x0)) of the quadrature
    from 0 to x; search / solve: the x that exp(scaling) (h_0 + F(x)) sends to the target (= the case's x), dimension 0 (solve-block:
    all dimensions); the solves also return f(x) and the status words."""
    import torch
    from umnn_amd import integral as I
    from umnn_amd.nets import mlp_spec
    net, x, h, scaling = (t.to(dev) for t in inputs(c))
    spec, n = mlp_spec(net), c["n"]
    with _lib.options(**c["options"]):
        if c["kind"] == FORWARD:
            return tuple(I.hip_forward(spec, None, x, h, n))
        if c["kind"] == SEARCH:
            out = torch.zeros_like(x)
            assert I.hip_invert_dim(spec, h, x, scaling, n, 0, SEARCH_ROUNDS, out)
            return (out[:, 0].clone(),)
        if c["kind"] == SOLVE:
            out, fx, status = I.hip_solve(spec, h, x, n, j=0, scaling=scaling, off_h0=True, max_iter=32)
            return out[:, 0].clone(), fx, status
        return tuple(I.hip_solve_block(spec, h, x, n, scaling=scaling, off_h0=True, max_iter=32))
