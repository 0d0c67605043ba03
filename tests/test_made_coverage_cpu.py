"""tests/_made_coverage_cases.py proved without a GPU: the restated launcher rules name both fused and all nine linear kernels over
the case tables (every name expected somewhere, none that is not instantiated); the emulated arithmetic is tied to pack_fragments' own
pieces and the float64 MLP to the pinned oracle; the input conditions the bounds rest on hold; and every entry reports its argument
errors before it touches a device."""
import ctypes

import numpy as np
import pytest
import torch

from oracle import cc_oracle as O
from tests import _made_coverage_cases as C
from umnn_amd import _lib
from umnn_amd.made import pack_fragments

FUSED_IDS = [c["id"] for c in C.FUSED]


# ---- names ------------------------------------------------------------------------------------------------------------------------------
def test_fused_names_at_256_cus():
    assert C.fused_threshold(256) == 8129
    assert C.fused_name(8128, 256) == "made_fused<RT=1>" and C.fused_name(8129, 256) == "made_fused<RT=4>"
    for c in C.FUSED:
        assert C.fused_name(C.fused_B(c, C.CUS_REF), C.CUS_REF) == c["name256"], c["id"]
    assert {c["name256"] for c in C.FUSED} == set(C.FUSED_NAMES)
    # (8129 - 1) % 64 == 0: the last workgroup of the RT = 4 launch holds one row
    assert (C.fused_threshold(256) - 1) % 64 == 0


def test_linear_names_at_256_cus():
    assert len(C.LINEAR_NAMES) == len(set(C.LINEAR_NAMES)) == 9
    expected = set()
    for rt, fg, name in C.LINEAR_FORCED:
        got, RT, G, TG = C.linear_plan(C.LINEAR_B, 1000, rt, fg, C.CUS_REF)
        assert got == name and RT == rt, (rt, fg)
        assert C.linear_plan(C.LINEAR_B, 1000, rt, fg, 8)[0] == name            # forced: no dependence on the CU count
        expected.add(name)
    for N in (1, 17, 64):
        for rt, fg, name in C.LINEAR_FORCED_SMALL:
            assert C.linear_plan(C.LINEAR_B, N, rt, fg, C.CUS_REF)[0] == name, (N, rt, fg)
    assert C.linear_plan(C.LINEAR_B, 1000, 0, 0, C.CUS_REF) == (C.LINEAR_AUTO_256, 1, 15, 5)
    assert expected == set(C.LINEAR_NAMES)
    # the tile counts of the three launch rules: TG <= 4, 5..8, > 8, > 16 at TPC = 2, and a group count above the tile count
    tgs = {(fg, C.linear_plan(C.LINEAR_B, 1000, 1, fg, C.CUS_REF)[3]) for _, fg, _ in C.LINEAR_FORCED}
    assert tgs == {(16, 4), (500, 1), (8, 8), (3, 21), (1, 63)}
    assert C.linear_plan(C.LINEAR_B, 1000, 1, 500, C.CUS_REF)[2] == 63
    # ring refills: more K-steps than PD only at PD = 8
    assert -(-257 // 32) == 9 and -(-512 // 32) == 16 and -(-C.LINEAR_EXACT_K // 32) > 8


# ---- truths -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,K", [(17, 31), (100, 257), (513, 512), (1, 1)])
def test_emu_from_the_packed_fragments_is_emu_from_the_plain_split(N, K):
    gen = torch.Generator().manual_seed(N + K)
    W, b = C.random_layer(N, K, gen)
    x = 2 * torch.randn(19, K, generator=gen)
    Wh, Wl = C.unpack_fragments(pack_fragments(W), N, K)
    ph, pl = C.split(W)
    assert torch.equal(Wh, ph) and torch.equal(Wl, pl)
    for relu in (0, 1):
        assert torch.equal(C.emu_layer(x, W, b, relu, pieces=(Wh, Wl)), C.emu_layer(x, W, b, relu))


@pytest.mark.parametrize("c", C.FUSED, ids=FUSED_IDS)
def test_chain_truths_and_input_conditions(c):
    for r in range(c["shifts"]):
        Ws, bs, x = C.fused_inputs(c, C.CUS_REF, r)
        ex = C.exact_chain(Ws, bs, x)
        ref = O.made_forward(C.as_numpy64(Ws), C.as_numpy64(bs), [np.ones(W.shape) for W in Ws], x.double().numpy())
        scale = float(ex.abs().max())
        assert np.abs(ex.numpy() - ref).max() <= 1e-12 * max(scale, 1.0)
        emu = C.emu_chain(Ws, bs, x)
        if c["kind"] == "exact":
            assert torch.equal(emu, ex) and torch.equal(ex, ex.round()) and scale < 2 ** 16
            assert all(int((W != 0).sum(1).max()) <= 2 and set(W.unique().tolist()) <= {-1.0, 0.0, 1.0} for W in Ws)
            assert scale > 0
        else:
            assert float((emu - ex).abs().max()) < C.EMU_CHAIN * scale, float((emu - ex).abs().max()) / scale


def test_exact_weights_visit_every_fragment_position():
    """Over the shifts of a case every (output tile, K-step, lane group, slot) -- every (tile, k) pair -- carries a non-zero weight."""
    for c in C.FUSED:
        if c["kind"] != "exact":
            continue
        for l in range(len(c["widths"]) - 1):
            K, N = c["widths"][l], c["widths"][l + 1]
            assert c["shifts"] >= -(-K // 32) or l > 0, c["id"]
            seen = sum((C.exact_weight(N, K, r) != 0).float() for r in range(-(-K // 32)))
            full = -(-N // 16) - (1 if N % 16 else 0)                  # a partial last tile has fewer than sixteen rows to spend
            tiles = seen[:16 * full].view(full, 16, K).sum(1) if full else seen[:0]
            assert bool((tiles > 0).all()), (c["id"], l)
    K = C.LINEAR_EXACT_K
    seen = sum((C.exact_weight(1000, K, r) != 0).float() for r in range(-(-K // 32)))
    assert bool((seen[:992].view(62, 16, K).sum(1) > 0).all())


def test_single_layer_e32_stays_small():
    """M x E32 must be the bound that binds: far below the whole-chain 2e-5 on every single layer of the linear table."""
    for K in C.LINEAR_KS:
        W, b, x = C.linear_inputs(K)
        for relu in (0, 1):
            emu, E32 = C.layer_truth(x, W, b, relu)
            assert C.M * E32 < 0.25 * C.WHOLE_CHAIN, (K, relu, E32)


def test_tables_cover_every_size_at_which_a_kernel_takes_another_path():
    Bs = {c["B"] for c in C.FUSED}
    assert {1, 15, 16, 17, 63, 64, 65, "thr", "thr-1"} <= Bs
    assert {len(c["widths"]) - 1 for c in C.FUSED} >= {1, 2, 3, 8}
    assert {c["widths"][0] for c in C.FUSED} >= {1, 31, 32, 33, 63, 512}
    assert {w for c in C.FUSED for w in c["widths"][1:-1]} >= {1, 15, 16, 17, 33, 48, 100, 500, 512}
    assert {c["widths"][-1] for c in C.FUSED} >= {1, 17, 512, 513, 1025}
    assert {w for c in C.FUSED for w in c["widths"][1:]} >= set(C.MODE2_WIDTHS)
    assert all(max(c["widths"]) <= 48 for c in C.FUSED if isinstance(c["B"], str))
    for d in C.GLUE_DS:
        nis = [B * d for B in C.glue_Bs(d)]
        assert min(nis) <= 255 and any(n > 256 for n in nis) and {1, 3, 4, 5} <= set(C.glue_Bs(d)), d
    assert any(B * 1 == 256 for B in C.glue_Bs(1)) and any(B * 64 == 256 for B in C.glue_Bs(64))
    # operand loads: 16-byte ones with one block and with two (K1 = 4, K - 4), scalar ones by an odd K, an odd K1 (1, K - 1) and --
    # in the GPU test -- by a view one float into a larger buffer
    vec = {(K, K1): C.linear_vec(K, K1) for K in C.LINEAR_KS for K1 in [None] + C.linear_k1s(K)}
    assert vec[(256, None)] and vec[(512, 4)] and vec[(256, 252)] and not vec[(256, 1)] and not vec[(512, 511)] and not vec[(257, None)]
    assert not C.linear_vec(256, None, aligned=False)
    assert all(set(C.linear_k1s(K)) == {1, 4, K - 4, K - 1} for K in C.LINEAR_KS if K >= 31)
    # both branches of the ReLU-backward kernel (N % 4 == 0 or not), several column blocks, a last block with idle lanes
    assert {N % 4 == 0 for N in C.RB_NS} == {True, False} and max(C.RB_NS) > 3 * 256 and any(N % 256 for N in C.RB_NS if N > 256)
    assert {N for _, N in C.RB_SHAPES} == set(C.RB_NS) and {B for B, _ in C.RB_SHAPES} == set(C.RB_BS)
    rows, cols, _ = C.split3_shapes(256)[0]
    assert rows == 4200 and rows * (cols // 2) > 16 * 256 * 256


# ---- argument errors: reported before anything is launched -------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def host():
    """A host buffer whose address stands in for device pointers the entries must never reach."""
    buf = (ctypes.c_float * 64)()
    return ctypes.c_void_p(ctypes.addressof(buf)), buf


def _fails(rc, what):
    lib = _lib.lib()
    assert rc != 0 and what in lib.umnn_last_error().decode(), (rc, lib.umnn_last_error())


def test_made_mlp_argument_errors(host):
    lib = _lib.lib()
    p, _ = host
    n0 = lib.umnn_made_launch_count()

    def call(widths, L=None, B=4, mode=0, ld=0, net=True):
        m = C.made_net(widths, [p.value] * 8, [p.value] * 8, L)
        return lib.umnn_made_mlp_forward_ex(ctypes.byref(m) if net else None, p, B, p, mode, ld, None)
    _fails(call([4, 4], net=False), "made_mlp")
    _fails(call([4, 4], L=0), "made_mlp")
    _fails(call([4] * 9, L=9), "made_mlp")
    _fails(call([4, 0, 4]), "made_mlp")
    _fails(call([0, 4]), "made_mlp")
    _fails(call([4, 513, 4]), "made_mlp")
    _fails(call([513, 4]), "made_mlp")
    _fails(call([4, 4], mode=3), "made_mlp")
    _fails(call([4, 4], mode=-1), "made_mlp")
    _fails(call([4, 4], mode=2, ld=3 * 4 + 1), "made_mlp")
    _fails(call([4, 4], B=-1), "made_mlp")
    assert call([4, 4], B=0) == 0 and call([4, 4], B=0, mode=2, ld=16) == 0
    assert lib.umnn_made_launch_count() == n0


def test_made_linear_argument_errors(host):
    lib = _lib.lib()
    p, _ = host
    n0 = lib.umnn_made_launch_count()

    def call(K=200, N=100, x2=None, K1=0, B=4, rt=0, fg=0, W=p, b=p, x=p, out=p):
        return lib.umnn_made_linear_forward(W, b, K, N, x, x2, K1, B, 0, out, 0, rt, fg, None)
    for bad in [dict(K=513), dict(K=0), dict(N=0), dict(rt=3), dict(rt=8), dict(fg=-1), dict(fg=65536), dict(x2=p, K1=200), dict(x2=p, K1=0),
                dict(B=-1), dict(W=None), dict(b=None), dict(x=None), dict(out=None)]:
        _fails(call(**bad), "made_linear")
    assert call(B=0) == 0
    assert lib.umnn_made_launch_count() == n0


def test_made_split3_argument_errors(host):
    lib = _lib.lib()
    p, _ = host
    _fails(lib.umnn_made_split3(p, 1, 4, 0, p, 13, None), "made_split3")
    _fails(lib.umnn_made_split3(p, 1, 0, 0, p, 16, None), "made_split3")
    _fails(lib.umnn_made_split3(p, -1, 4, 0, p, 16, None), "made_split3")
    _fails(lib.umnn_made_split3(None, 1, 4, 0, p, 16, None), "made_split3")
    assert lib.umnn_made_split3(p, 0, 4, 0, p, 16, None) == 0


def test_relu_bwd_bias_argument_errors(host):
    lib = _lib.lib()
    p, _ = host
    _fails(lib.umnn_made_relu_bwd_bias(p, p, 4, 0, p, 1, p, None), "made_relu_bwd_bias")
    _fails(lib.umnn_made_relu_bwd_bias(p, p, 4, 8, p, 0, p, None), "made_relu_bwd_bias")
    _fails(lib.umnn_made_relu_bwd_bias(p, p, -1, 8, p, 1, p, None), "made_relu_bwd_bias")
    _fails(lib.umnn_made_relu_bwd_bias(p, p, 4, 8, p, 1, None, None), "made_relu_bwd_bias")
    _fails(lib.umnn_made_relu_bwd_bias(None, p, 4, 8, p, 1, p, None), "made_relu_bwd_bias")
    _fails(lib.umnn_made_relu_bwd_bias(p, p, 4, 8, None, 1, p, None), "made_relu_bwd_bias")
    for B, N in [(0, 4), (-3, 4), (4, 0)]:
        assert lib.umnn_made_relu_bwd_bias_row_blocks(B, N) == 1


def test_glue_argument_errors(host):
    lib = _lib.lib()
    p, _ = host
    cot = lambda B=4, d=3, gz=p, glj=p, fx=p, s=p, gF=p, gfx=p: lib.umnn_flow_block_cotangents(gz, glj, fx, s, B, d, 1, gF, gfx, None)  # noqa: E731
    for bad in [dict(d=0), dict(B=-1), dict(s=None), dict(gF=None), dict(fx=None)]:
        _fails(cot(**bad), "flow cotangents")
    assert cot(B=0) == 0
    fwd = lambda B=4, d=3, z=p, lj=p, ll=p: lib.umnn_flow_ll_forward(z, lj, B, d, ll, None)                                             # noqa: E731
    for bad in [dict(d=0), dict(B=-1), dict(z=None), dict(lj=None), dict(ll=None)]:
        _fails(fwd(**bad), "flow ll")
    assert fwd(B=0) == 0
    bwd = lambda B=4, d=3, z=p, g=p: lib.umnn_flow_ll_backward(z, g, B, d, p, p, None)                                                  # noqa: E731
    for bad in [dict(d=0), dict(B=-1), dict(z=None), dict(g=None)]:
        _fails(bwd(**bad), "flow ll backward")
    assert bwd(B=0) == 0
