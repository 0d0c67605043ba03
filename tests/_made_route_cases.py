"""The conditioner's route table, written out by hand: inputs of ``umnn_amd.made.conditioner_route`` and the record it must return.

Nothing here is computed by the code under test.  ``DEFAULTS`` are the switches with no environment variable set.  Per case:
  rows, widths [(in_features, out_features) per masked linear], n_out (the output width that survives), the flags of the call
  (``FLAGS`` where not given), ``opts`` (switches that differ from DEFAULTS) and ``expect`` = (route name, the two blocks are read
  without the cat, the output layer goes to the library GEMM).
  ``gpu``: how tests/test_gpu_made_routes.py reaches the case with ``raw`` on a device, or None where it cannot (with the reason):
    net ("MADE", nin, hidden, nout) | ("COND", nin, cond_in, hidden, nout) -- its masked linears have the widths of the case;
    fast / fused: arguments of set_made_fast_path / set_made_fused (fused: a dict of keyword arguments besides ``enabled=True``);
    train_fused: the switch of the one-node training chain; grad: run under autograd; autocast: under bf16 autocast (the chain
    it is compared with too); frozen: nothing requires grad; double: fp64 weights and input; x_dtype / ctx_dtype: of the inputs.
The launches a route makes (``LAUNCHES``): none that the conditioner's launch counter sees for the library-GEMM and F.linear routes
(the split launch is not counted), one ``made_fused`` launch for "fused" and "hybrid", one ``made_linear`` launch per masked linear
for "layered", less one when the output layer goes to the library."""

DEFAULTS = dict(fast=True, fused=True, max_rows=32768, wide_out=False, hybrid=False, layered=True, layered_max_rows=32768,
                layered_lib_out_rows=4096, train_fused=True, addmm_act=True)
FLAGS = dict(cuda_fp32=True, two_fp32_blocks=False, grad=False, needs_grad=False, autocast=False, graph=False, probe=True)

NARROW = ("MADE", 5, [33], 15)                       # widths [(5, 33), (33, 15)]
WIDE = ("MADE", 20, [37], 600)                       # widths [(20, 37), (37, 600)]
WIDE_COND = ("COND", 20, 12, [37], 960)              # widths [(32, 37), (37, 960)], 20 * 30 = 600 columns survive
W_NARROW, W_WIDE, W_WIDE_COND = [(5, 33), (33, 15)], [(20, 37), (37, 600)], [(32, 37), (37, 960)]
W_WIDE3, W_WIDE3_COND = [(20, 37), (37, 37), (37, 600)], [(32, 37), (37, 37), (37, 960)]


def _case(id, expect, rows=19, widths=W_NARROW, n_out=15, opts=None, gpu=None, **flags):
    return dict(id=id, rows=rows, widths=widths, n_out=n_out, flags={**FLAGS, **flags}, opts=opts or {}, expect=expect, gpu=gpu)


CASES = [
    # ---- off the fast path
    _case("recorded graph", ("graph", False, False), graph=True, gpu=None),          # (raw under a compiler: tests/test_gpu_torch_compile.py)
    _case("recorded graph, training", ("graph", False, False), graph=True, grad=True, needs_grad=True, gpu=None),
    _case("CPU input", ("linear", False, False), cuda_fp32=False, gpu=None),         # (not a device call)
    _case("fp64 input", ("linear", False, False), cuda_fp32=False, gpu=dict(net=NARROW, double=True)),
    _case("fast path switched off", ("linear", False, False), opts=dict(fast=False), gpu=dict(net=NARROW, fast=False)),
    _case("fast path switched off, ConditionnalMADE", ("linear", False, False), widths=W_WIDE_COND, n_out=600, two_fp32_blocks=True,
          opts=dict(fast=False), gpu=dict(net=WIDE_COND, fast=False)),
    _case("probe false", ("linear", False, False), probe=False, gpu=None),           # (a GPU box has torch.mm(out_dtype=))
    _case("grad on, something requires grad", ("train", False, False), grad=True, needs_grad=True, gpu=dict(net=NARROW, grad=True)),
    _case("grad on, ConditionnalMADE", ("train", False, False), widths=W_WIDE_COND, n_out=600, two_fp32_blocks=True, grad=True,
          needs_grad=True, gpu=dict(net=WIDE_COND, grad=True)),
    _case("grad on, nothing requires grad", ("linear", False, False), grad=True, gpu=dict(net=NARROW, grad=True, frozen=True)),
    _case("grad on, one-node chain switched off", ("linear", False, False), grad=True, needs_grad=True, opts=dict(train_fused=False),
          gpu=dict(net=NARROW, grad=True, train_fused=False)),
    # (autocast runs the F.linear GEMMs in bf16: the device test compares with the same chain under the same autocast)
    _case("grad on under autocast", ("linear", False, False), grad=True, needs_grad=True, autocast=True,
          gpu=dict(net=NARROW, grad=True, autocast=True)),
    _case("grad on, host input", ("linear", False, False), cuda_fp32=False, grad=True, needs_grad=True, gpu=None),      # (not a device call)
    # ---- the fast path: split + library GEMM per layer
    _case("fused off", ("split", False, False), opts=dict(fused=False), gpu=dict(net=NARROW, fused_enabled=False)),
    _case("fused off, wide output", ("split", False, False), widths=W_WIDE, n_out=600, opts=dict(fused=False),
          gpu=dict(net=WIDE, fused_enabled=False)),
    _case("rows at max_rows", ("fused", False, False), rows=16, opts=dict(max_rows=16), gpu=dict(net=NARROW, fused=dict(max_rows=16))),
    _case("rows at max_rows + 1", ("split", False, False), rows=17, opts=dict(max_rows=16), gpu=dict(net=NARROW, fused=dict(max_rows=16))),
    _case("8 layers", ("fused", False, False), widths=[(5, 8)] + [(8, 8)] * 6 + [(8, 15)], gpu=dict(net=("MADE", 5, [8] * 7, 15))),
    _case("9 layers", ("split", False, False), widths=[(5, 8)] + [(8, 8)] * 7 + [(8, 15)], gpu=dict(net=("MADE", 5, [8] * 8, 15))),
    _case("in_features 512", ("fused", False, False), widths=[(5, 512), (512, 16), (16, 15)], gpu=dict(net=("MADE", 5, [512, 16], 15))),
    _case("in_features 513", ("split", False, False), widths=[(5, 513), (513, 16), (16, 15)], gpu=dict(net=("MADE", 5, [513, 16], 15))),
    _case("in_features 513, wide output", ("split", False, False), widths=[(20, 513), (513, 16), (16, 600)], n_out=600,
          gpu=dict(net=("MADE", 20, [513, 16], 600))),
    # ---- the whole MLP in one launch
    _case("narrow", ("fused", False, False), gpu=dict(net=NARROW)),
    _case("surviving width 512", ("fused", False, False), widths=[(16, 37), (37, 512)], n_out=512, gpu=dict(net=("MADE", 16, [37], 512))),
    _case("surviving width 513", ("layered", False, False), widths=[(27, 37), (37, 513)], n_out=513, gpu=dict(net=("MADE", 27, [37], 513))),
    _case("ConditionnalMADE, full output 640 > 512, 400 survive", ("fused", False, False), widths=[(32, 37), (37, 640)], n_out=400,
          two_fp32_blocks=True, gpu=dict(net=("COND", 20, 12, [37], 640))),
    _case("wide_out", ("fused", False, False), widths=W_WIDE, n_out=600, opts=dict(wide_out=True), gpu=dict(net=WIDE, fused=dict(wide_out=True))),
    _case("wide_out, ConditionnalMADE", ("fused", False, False), widths=W_WIDE_COND, n_out=600, two_fp32_blocks=True, opts=dict(wide_out=True),
          gpu=dict(net=WIDE_COND, fused=dict(wide_out=True))),
    _case("wide_out wins over hybrid", ("fused", False, False), widths=W_WIDE, n_out=600, opts=dict(wide_out=True, hybrid=True),
          gpu=dict(net=WIDE, fused=dict(wide_out=True, hybrid=True))),
    # ---- the hidden stack in one launch + one library GEMM
    _case("hybrid, one layer", ("layered", False, False), widths=[(20, 600)], n_out=600, opts=dict(hybrid=True),
          gpu=dict(net=("MADE", 20, [], 600), fused=dict(hybrid=True))),
    _case("hybrid, two layers", ("hybrid", False, False), widths=W_WIDE, n_out=600, opts=dict(hybrid=True), gpu=dict(net=WIDE, fused=dict(hybrid=True))),
    _case("hybrid, two hidden layers", ("hybrid", False, False), widths=W_WIDE3, n_out=600, opts=dict(hybrid=True),
          gpu=dict(net=("MADE", 20, [37, 37], 600), fused=dict(hybrid=True))),
    _case("hybrid, two hidden layers, ConditionnalMADE", ("hybrid", False, False), widths=W_WIDE3_COND, n_out=600, two_fp32_blocks=True,
          opts=dict(hybrid=True), gpu=dict(net=("COND", 20, 12, [37, 37], 960), fused=dict(hybrid=True))),
    _case("hybrid, narrow output", ("fused", False, False), opts=dict(hybrid=True), gpu=dict(net=NARROW, fused=dict(hybrid=True))),
    # ---- one launch per masked linear
    _case("wide output", ("layered", False, False), widths=W_WIDE, n_out=600, gpu=dict(net=WIDE)),
    _case("wide output, two hidden layers", ("layered", False, False), widths=W_WIDE3, n_out=600, gpu=dict(net=("MADE", 20, [37, 37], 600))),
    _case("layered off", ("split", False, False), widths=W_WIDE, n_out=600, opts=dict(layered=False), gpu=dict(net=WIDE, fused=dict(layered=False))),
    _case("rows at the library-output limit", ("layered", False, False), rows=4096, widths=W_WIDE, n_out=600, gpu=dict(net=WIDE)),
    _case("rows above the library-output limit", ("layered", False, True), rows=4097, widths=W_WIDE, n_out=600, gpu=dict(net=WIDE)),
    _case("rows above the library-output limit, ConditionnalMADE", ("layered", True, True), rows=4097, widths=W_WIDE_COND, n_out=600,
          two_fp32_blocks=True, gpu=dict(net=WIDE_COND)),
    # (the surviving width decides the route, the layer's full out_features whether its GEMM goes to the library)
    _case("above the library-output limit, output layer 513 wide", ("layered", False, True), rows=4097,
          widths=[(27, 37), (37, 513)], n_out=513, gpu=dict(net=("MADE", 27, [37], 513))),
    _case("above the library-output limit, output layer 512 wide", ("layered", False, False), rows=4097, widths=[(27, 37), (37, 512)], n_out=513,
          gpu=None),                                                                    # (no module has such widths: the rule alone)
    _case("single layer above the library-output limit", ("layered", False, False), rows=4097, widths=[(20, 600)], n_out=600,
          gpu=dict(net=("MADE", 20, [], 600))),
    _case("rows at the layered limit", ("layered", False, True), rows=32768, widths=W_WIDE, n_out=600, opts=dict(max_rows=65536),
          gpu=dict(net=WIDE, fused=dict(max_rows=65536))),
    _case("rows above the layered limit", ("split", False, False), rows=32769, widths=W_WIDE, n_out=600, opts=dict(max_rows=65536),
          gpu=dict(net=WIDE, fused=dict(max_rows=65536))),
    _case("rows above max_rows, wide output", ("split", False, False), rows=32769, widths=W_WIDE, n_out=600, gpu=dict(net=WIDE)),
    # ---- ConditionnalMADE's two blocks: read without the cat on the per-layer-kernel route only, and only all-fp32
    _case("two fp32 blocks", ("layered", True, False), widths=W_WIDE_COND, n_out=600, two_fp32_blocks=True, gpu=dict(net=WIDE_COND)),
    _case("fp32 x, bf16 context (widened: two fp32 blocks)", ("layered", True, False), widths=W_WIDE_COND, n_out=600, two_fp32_blocks=True,
          gpu=dict(net=WIDE_COND, ctx_dtype="bfloat16")),
    _case("bf16 x, fp32 context (cat, then widened)", ("layered", False, False), widths=W_WIDE_COND, n_out=600, two_fp32_blocks=False,
          gpu=dict(net=WIDE_COND, x_dtype="bfloat16")),
    _case("two fp32 blocks, layered off", ("split", False, False), widths=W_WIDE_COND, n_out=600, two_fp32_blocks=True, opts=dict(layered=False),
          gpu=dict(net=WIDE_COND, fused=dict(layered=False))),
    _case("two fp32 blocks, recorded graph", ("graph", False, False), widths=W_WIDE_COND, n_out=600, two_fp32_blocks=True, graph=True, gpu=None),
]

# route name -> (conditioner launches as a function of (masked linears, output layer on the library), kernel name of the last one)
LAUNCHES = {
    "graph": (lambda n, lib_out: 0, None), "linear": (lambda n, lib_out: 0, None), "train": (lambda n, lib_out: 0, None),
    "split": (lambda n, lib_out: 0, None),
    "fused": (lambda n, lib_out: 1, "made_fused"), "hybrid": (lambda n, lib_out: 1, "made_fused"),
    "layered": (lambda n, lib_out: n - 1 if lib_out else n, "made_linear"),
}
