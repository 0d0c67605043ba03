"""Every conditioner kernel (made_fused<RT=1|4>, the nine made_linear variants, split3), the ReLU-backward / bias-gradient kernels and
the training glue, called through the C entries on the cases of tests/_made_coverage_cases.py: float64 truths with bounds from the
reference's own float32 error, exact-integer cases with no tolerance, bit-equalities between variants, NaN-prefilled outputs with a
guard region behind each.  The measured ratios are printed (``pytest -s``) and recorded in profiles/made_coverage/README.md."""
import ctypes
import types

import pytest
import torch

from tests import _made_coverage_cases as C
from umnn_amd import _lib
from umnn_amd.made import pack_fragments

pytestmark = pytest.mark.gpu
NAN = float("nan")


@pytest.fixture(scope="module")
def G():
    assert torch.cuda.is_available()
    dev = torch.device("cuda:0")
    return types.SimpleNamespace(dev=dev, lib=_lib.lib(), stream=ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream),
                                 cus=torch.cuda.get_device_properties(dev).multi_processor_count)


def biteq(a, b):
    """Same shape, dtype and bit pattern (NaN-prefilled elements that were never written differ from any expected value)."""
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    it = {2: torch.int16, 4: torch.int32, 8: torch.int64}[a.element_size()]
    return bool(torch.equal(a.contiguous().view(it), b.contiguous().view(it))) and not bool(torch.isnan(a).any())


def guarded(n, dtype, dev):
    """A NaN-filled buffer of n elements with C.GUARD more behind it."""
    return torch.full((n + C.GUARD,), NAN, dtype=dtype, device=dev)


def untouched(buf, n):
    return bool(torch.isnan(buf[n:]).all())


def note(what, ratio):
    print(f"[made-coverage] {what} err/E32 = {ratio:.3f}")


# ---- part 1: made_fused -----------------------------------------------------------------------------------------------------------------
def mlp(G, widths, frags, bd, x, L, mode=0, ld=0):
    """umnn_made_mlp_forward_ex on the depth-L prefix -> (output [B, N] or [B, ld], kernel name)."""
    B, N = x.shape[0], widths[L]
    n = B * (ld if mode == 2 else N)
    buf = guarded(n, torch.float32 if mode == 0 else torch.bfloat16, G.dev)
    net = C.made_net(widths, [f.data_ptr() for f in frags], [b.data_ptr() for b in bd], L)
    _lib.check(G.lib.umnn_made_mlp_forward_ex(ctypes.byref(net), x.data_ptr(), B, buf.data_ptr(), mode, ld, G.stream), "made_mlp")
    assert untouched(buf, n), "wrote behind the output"
    return buf[:n].view(B, -1), G.lib.umnn_last_made_kernel_name().decode()


def split3(G, x, relu, ld):
    rows, cols = x.shape
    buf = guarded(rows * ld, torch.bfloat16, G.dev)
    _lib.check(G.lib.umnn_made_split3(x.data_ptr(), rows, cols, relu, buf.data_ptr(), ld, G.stream), "split3")
    assert untouched(buf, rows * ld)
    return buf[:rows * ld].view(rows, ld)


@pytest.mark.parametrize("c", C.FUSED, ids=[c["id"] for c in C.FUSED])
def test_fused_kernel(G, c):
    widths, B = c["widths"], C.fused_B(c, G.cus)
    L = len(widths) - 1
    want_name = C.fused_name(B, G.cus)
    for r in range(c["shifts"]):
        Ws, bs, x = C.fused_inputs(c, G.cus, r)
        frags, bd, xd = [pack_fragments(W.to(G.dev)) for W in Ws], [b.to(G.dev) for b in bs], x.to(G.dev)
        outs = []
        for l in range(1, L + 1):
            o, name = mlp(G, widths, frags, bd, xd, l)
            assert name == want_name
            outs.append(o)
        full = outs[-1]
        assert biteq(mlp(G, widths, frags, bd, xd, L)[0], full), "a second launch differs"
        assert biteq(mlp(G, widths, frags, bd, xd, L, mode=1)[0], full.bfloat16()), "mode 1 is not mode 0 rounded to bf16"
        if want_name == C.FUSED_NAMES[1]:
            # the per-element accumulation order does not depend on RT: rows 0..63 against a launch of those rows alone
            o64, name = mlp(G, widths, frags, bd, xd[:64].contiguous(), L)
            assert name == C.fused_name(64, G.cus) and biteq(full[:64], o64)
        ex = C.exact_chain(Ws, bs, x)
        if c["kind"] == "exact":
            for l in range(1, L + 1):
                assert torch.equal(outs[l - 1].double().cpu(), C.exact_chain(Ws[:l], bs[:l], x)), (r, l)
            continue
        scale = float(ex.abs().max())
        whole = float((full.double().cpu() - ex).abs().max()) / scale
        print(f"[made-coverage] {want_name} {c['id']} whole chain {whole:.2e}")
        assert whole <= C.WHOLE_CHAIN
        for l in range(1, L + 1):
            # peeling: layer l of the depth-l prefix against emu of layer l on the kernel's own depth-(l-1) pre-activation
            emu, E32 = C.layer_truth(x if l == 1 else outs[l - 2], Ws[l - 1], bs[l - 1], l > 1)
            ratio = C.layer_ratio(outs[l - 1], emu, E32)
            note(f"{want_name} {c['id']} layer {l} ({widths[l - 1]}x{widths[l]})", ratio)
            assert ratio <= C.M, (l, ratio, E32)
        for l in range(1, L + 1):
            # what peeling rests on: a stored hidden value is the re-split one.  Mode 2 of a prefix = split3(relu) of its mode 0
            N = widths[l]
            if N > 512:
                continue
            for ld in (C.pad8(3 * N + 2), C.pad8(3 * N + 2) + 24):
                m2, _ = mlp(G, widths, frags, bd, xd, l, mode=2, ld=ld)
                assert biteq(m2, split3(G, outs[l - 1], 1, ld)), (l, ld)
                assert biteq(m2, C.split3_torch(outs[l - 1], 1, ld)), (l, ld)       # (ones at 3N, 3N + 1; zeros to ld)


def test_fused_mode2_widths_are_covered():
    """test_fused_kernel runs mode 2 on every prefix of width <= 512: the widths the operand format is held to are among them."""
    assert set(C.MODE2_WIDTHS) <= {w for c in C.FUSED if c["kind"] == "random" for w in c["widths"][1:] if w <= 512}


@pytest.mark.parametrize("cond", [0, 11])
def test_fused_kernel_is_exactly_autoregressive(G, cond):
    """Through MADE.raw / ConditionnalMADE.raw on hidden widths that are no multiple of 16: outputs of dimensions <= j do not move at
    all when x[:, j:] changes."""
    from umnn_amd import MADE, ConditionnalMADE
    torch.manual_seed(5)
    nin, E, B = 7, 3, 37
    made = (ConditionnalMADE(nin, cond, [50, 37], (nin + cond) * E, num_masks=1, natural_ordering=True) if cond
            else MADE(nin, [50, 37], nin * E, num_masks=1, natural_ordering=True)).to(G.dev).eval()
    x = torch.randn(B, nin, device=G.dev)
    ctx = (torch.randn(B, cond, device=G.dev),) if cond else ()
    with torch.no_grad():
        n0 = G.lib.umnn_made_launch_count()
        h = made.raw(x, *ctx).view(B, E, nin)
        assert G.lib.umnn_made_launch_count() > n0 and G.lib.umnn_last_made_kernel_name().decode() == C.fused_name(B, G.cus), \
            "the one-launch conditioner kernel did not run"
        for j in range(nin):
            x2 = x.clone()
            x2[:, j:] = torch.randn(B, nin - j, device=G.dev) * 3
            h2 = made.raw(x2, *ctx).view(B, E, nin)
            assert biteq(h[:, :, :j + 1], h2[:, :, :j + 1]), j
            assert j + 1 == nin or not torch.equal(h, h2)


# ---- part 2: made_linear ----------------------------------------------------------------------------------------------------------------
def linear(G, frag, b, K, N, x, x2, K1, relu, bf16, rt, fg):
    B = x.shape[0]
    buf = guarded(B * N, torch.bfloat16 if bf16 else torch.float32, G.dev)
    _lib.check(G.lib.umnn_made_linear_forward(frag.data_ptr(), b.data_ptr(), K, N, x.data_ptr(), None if x2 is None else x2.data_ptr(), K1,
                                              B, relu, buf.data_ptr(), bf16, rt, fg, G.stream), "made_linear")
    assert untouched(buf, B * N), "wrote behind the output"
    return buf[:B * N].view(B, N), G.lib.umnn_last_made_kernel_name().decode()


def operand_forms(G, x, K):
    """[(tag, x, x2, K1)]: one block (16-byte loads when K % 4 == 0), the same one float into a larger buffer (scalar loads), and two
    blocks at every K1 of the table (16-byte loads iff K1 and K - K1 are multiples of 4)."""
    B = x.shape[0]
    big = torch.empty(B * K + 8, device=G.dev)
    off = big[1:1 + B * K].view(B, K)
    off.copy_(x)
    assert x.data_ptr() % 16 == 0 and off.data_ptr() % 16 == 4
    forms = [("one", x, None, 0), ("offset", off, None, 0)]
    for K1 in C.linear_k1s(K):
        x1, x2 = x[:, :K1].contiguous(), x[:, K1:].contiguous()
        assert x1.data_ptr() % 16 == 0 and x2.data_ptr() % 16 == 0
        forms.append((f"K1={K1}", x1, x2, K1))
    return forms


@pytest.mark.parametrize("K", C.LINEAR_KS)
def test_linear_kernel_variants(G, K):
    W, b, x = C.linear_inputs(K)
    B = C.LINEAR_B
    xd = x.to(G.dev)
    forms = operand_forms(G, xd, K)
    seen = set()
    for N in C.LINEAR_NS:
        Wn, bn = W[:N].contiguous(), b[:N].contiguous()
        frag, bd = pack_fragments(Wn.to(G.dev)), bn.to(G.dev)
        table = (C.LINEAR_FORCED if N == 1000 else C.LINEAR_FORCED_SMALL) + [(0, 0, C.linear_plan(B, N, 0, 0, G.cus)[0])]
        for relu in (0, 1):
            emu, E32 = C.layer_truth(x, Wn, bn, relu)
            ref = {}                                        # accumulators per tile (3 at TPC=1, 1 at TPC=2) -> first output
            for rt, fg, want_name in table:
                acc = 1 if "TPC=2" in want_name else 3
                for tag, xa, xb, K1 in forms:
                    out, name = linear(G, frag, bd, K, N, xa, xb, K1, relu, 0, rt, fg)
                    assert name == want_name, (N, rt, fg, tag)
                    if acc not in ref:
                        ref[acc] = out
                    # same accumulator count: the same bits across RT, G, NW, one block or two, vector or scalar operand loads
                    assert biteq(out, ref[acc]), (N, relu, rt, fg, tag)
                    if name not in seen:
                        seen.add(name)
                        ratio = C.layer_ratio(out, emu, E32)
                        note(f"{name} K={K} N={N} relu={relu}", ratio)
                        assert ratio <= C.M, (name, ratio, E32)
                o16, _ = linear(G, frag, bd, K, N, xd, None, 0, relu, 1, rt, fg)
                assert biteq(o16, ref[acc].bfloat16()), (N, relu, rt, fg)
                # fewer rows (one partial row group): the same bits per row
                o17, _ = linear(G, frag, bd, K, N, xd[:17].contiguous(), None, 0, relu, 0, rt, fg)
                assert biteq(o17, ref[acc][:17]), (N, relu, rt, fg)
            for acc, out in ref.items():
                # across the two accumulator counts only the per-layer bound holds (another summation order)
                ratio = C.layer_ratio(out, emu, E32)
                note(f"made_linear accumulators={acc} K={K} N={N} relu={relu}", ratio)
                assert ratio <= C.M, (acc, ratio, E32)
    assert seen >= set(C.LINEAR_NAMES)


def test_linear_kernel_exact_cases(G):
    """Integer inputs, weights in {-1, 0, 1} walked over every (tile, K-step) by the shift r: all nine variants must give the float64
    result exactly."""
    K, N, B = C.LINEAR_EXACT_K, 1000, C.LINEAR_B
    seen = set()
    for r in range(-(-K // 32)):
        (W,), (b,), x = C.exact_net([K, N], B, 5000 + r, r)
        frag, bd, xd = pack_fragments(W.to(G.dev)), b.to(G.dev), x.to(G.dev)
        relu = r & 1
        want = C.exact_layer(x, W, b, relu)
        assert torch.equal(C.emu_layer(x, W, b, relu), want)
        for rt, fg, want_name in C.LINEAR_FORCED:
            out, name = linear(G, frag, bd, K, N, xd, None, 0, relu, 0, rt, fg)
            assert name == want_name
            seen.add(name)
            assert torch.equal(out.double().cpu(), want), (r, rt, fg)
    assert seen == set(C.LINEAR_NAMES)


# ---- part 3: split3 ---------------------------------------------------------------------------------------------------------------------
def test_split3_grid_stride_loop(G):
    for rows, cols, relu in C.split3_shapes(G.cus):
        assert rows * ((cols + 1) // 2) > 16 * G.cus * 256          # more pairs than threads: the stride loop runs
        x = torch.randn(rows, cols, device=G.dev) * 5
        ld = C.pad8(3 * cols + 2)
        assert biteq(split3(G, x, relu, ld), C.split3_torch(x, relu, ld)), (rows, cols, relu)


# ---- part 4: ReLU backward + bias gradient ----------------------------------------------------------------------------------------------
def relu_bwd_bias(G, g, a, rb):
    """-> (g after the call, gb)."""
    B, N = g.shape
    gbuf, part, gb = guarded(B * N, torch.float32, G.dev), guarded(rb * N, torch.float32, G.dev), guarded(N, torch.float32, G.dev)
    gbuf[:B * N].copy_(g.reshape(-1))
    _lib.check(G.lib.umnn_made_relu_bwd_bias(gbuf.data_ptr(), None if a is None else a.data_ptr(), B, N, part.data_ptr(), rb, gb.data_ptr(),
                                             G.stream), "relu_bwd_bias")
    assert untouched(gbuf, B * N) and untouched(part, rb * N) and untouched(gb, N)
    return gbuf[:B * N].view(B, N), gb[:N]


@pytest.mark.parametrize("B,N", C.RB_SHAPES)
def test_relu_bwd_bias(G, B, N):
    auto = G.lib.umnn_made_relu_bwd_bias_row_blocks(B, N)
    assert 1 <= auto <= 64
    worst = 0.0
    for kind in ("exact", "random"):
        g, a = C.rb_inputs(B, N, kind)
        gd, ad = g.to(G.dev), a.to(G.dev)
        gy, s64, mag, E32 = C.rb_truth(g, a)
        _, s64n, magn, E32n = C.rb_truth(g, None)
        for rb in C.rb_row_blocks(B, auto):
            got_g, got_b = relu_bwd_bias(G, gd, ad, rb)
            # g . [a > 0] with a in {0, -0, positive}: the masked entries are +0 (what ReLU's backward writes; the product g * 0 would
            # carry the sign of g into the zero), every other one the untouched float
            assert biteq(got_g, gy.to(G.dev)), (kind, rb)
            assert torch.equal(got_g, gd * (ad > 0))
            nul_g, nul_b = relu_bwd_bias(G, gd, None, rb)
            assert biteq(nul_g, gd), (kind, rb)
            if kind == "exact":
                assert torch.equal(got_b.double().cpu(), s64) and torch.equal(nul_b.double().cpu(), s64n), rb
            else:
                for got, t64, m, e in ((got_b, s64, mag, E32), (nul_b, s64n, magn, E32n)):
                    ratio = float(((got.double().cpu() - t64).abs() / m).max()) / e
                    worst = max(worst, ratio)
                    assert ratio <= C.M, (rb, ratio, e)
                assert biteq(relu_bwd_bias(G, gd, ad, rb)[1], got_b), "a repeat differs"
    note(f"made_relu_bwd_bias {'vector' if N % 4 == 0 else 'scalar'} branch B={B} N={N}", worst)


# ---- part 5: training glue --------------------------------------------------------------------------------------------------------------
def cotangents(G, I, B, d, reverse, use_gz=True, use_glj=True, use_gfx=True):
    gF, gfx = guarded(B * d, torch.float32, G.dev), guarded(B * d, torch.float32, G.dev)
    _lib.check(G.lib.umnn_flow_block_cotangents(C.ptr(I["g_z"] if use_gz else None), C.ptr(I["g_lj"] if use_glj else None),
                                                C.ptr(I["f_x"] if use_glj else None), C.ptr(I["scaling"]), B, d, reverse, gF.data_ptr(),
                                                gfx.data_ptr() if use_gfx else None, G.stream), "cotangents")
    assert untouched(gF, B * d) and untouched(gfx, B * d if use_gfx else 0)
    return gF[:B * d].view(B, d), gfx[:B * d].view(B, d)


@pytest.mark.parametrize("d", C.GLUE_DS)
def test_flow_block_cotangents(G, d):
    worst = [0.0, 0.0]
    for B in C.glue_Bs(d):
        I = C.glue_inputs(B, d)
        Id = {k: v.to(G.dev) for k, v in I.items()}
        for reverse in (0, 1):
            tF, tfx, fF, ffx = C.cotangents_truth(I, reverse)
            gF, gfx = cotangents(G, Id, B, d, reverse)
            for i, (got, t64, f32) in enumerate(((gF, tF, fF), (gfx, tfx, ffx))):
                ratio = C.rel_ratio(got.cpu(), t64, f32)
                worst[i] = max(worst[i], ratio)
                assert ratio <= C.M, (B, reverse, i, ratio)
            z0, fx1 = cotangents(G, Id, B, d, reverse, use_gz=False)
            assert biteq(z0, torch.zeros_like(z0)) and biteq(fx1, gfx)                 # g_z null: gF exactly 0
            F1, z1 = cotangents(G, Id, B, d, reverse, use_glj=False)
            assert biteq(z1, torch.zeros_like(z1)) and biteq(F1, gF)                   # g_log_jac null: g_fx exactly 0
            F2, _ = cotangents(G, Id, B, d, reverse, use_gfx=False)
            assert biteq(F2, gF)                                                       # g_fx null: nothing but gF is written
    note(f"flow_block_cotangents d={d} gF", worst[0])
    note(f"flow_block_cotangents d={d} g_fx", worst[1])


def ll_forward(G, z, lj):
    B, d = z.shape
    ll = guarded(B, torch.float32, G.dev)
    _lib.check(G.lib.umnn_flow_ll_forward(z.data_ptr(), lj.data_ptr(), B, d, ll.data_ptr(), G.stream), "ll_forward")
    assert untouched(ll, B)
    return ll[:B]


@pytest.mark.parametrize("d", C.GLUE_DS)
def test_flow_ll_forward(G, d):
    worst = 0.0
    for B in C.glue_Bs(d):
        I = C.glue_inputs(B, d)
        t64, mag, f32 = C.ll_truth(I["z"], I["lj"])
        E32 = max(float(((f32.double() - t64).abs() / mag).max()), C.FLOOR)
        got = ll_forward(G, I["z"].to(G.dev), I["lj"].to(G.dev))
        ratio = float(((got.double().cpu() - t64).abs() / mag).max()) / E32
        worst = max(worst, ratio)
        assert ratio <= C.M, (B, ratio, E32)
        assert biteq(ll_forward(G, I["z"].to(G.dev), I["lj"].to(G.dev)), got)
    # position probes: one log_jac of 1024 at column 0, 63, 64 or d - 1 of an otherwise zero row; a dropped or doubled element shows whole
    z, lj, want = C.ll_probes(d)
    got = ll_forward(G, z.to(G.dev), lj.to(G.dev)).double().cpu()
    assert float((got - want).abs().max()) <= 8 * 2.0 ** -13, (got, want)         # eight ulps of 1024: at most ten roundings of half an ulp
    note(f"flow_ll_forward d={d}", worst)


@pytest.mark.parametrize("d", C.GLUE_DS)
def test_flow_ll_backward(G, d):
    for B in C.glue_Bs(d):
        I = C.glue_inputs(B, d)
        z, g = I["z"].to(G.dev), I["g_ll"].to(G.dev)
        want_z, want_lj = -z * g[:, None], g[:, None].expand(B, d).contiguous()
        for use_z, use_lj in ((1, 1), (0, 1), (1, 0)):
            gz, glj = guarded(B * d, torch.float32, G.dev), guarded(B * d, torch.float32, G.dev)
            _lib.check(G.lib.umnn_flow_ll_backward(z.data_ptr(), g.data_ptr(), B, d, gz.data_ptr() if use_z else None,
                                                   glj.data_ptr() if use_lj else None, G.stream), "ll_backward")
            assert untouched(gz, B * d if use_z else 0) and untouched(glj, B * d if use_lj else 0)
            assert not use_z or biteq(gz[:B * d].view(B, d), want_z), (B, use_z, use_lj)
            assert not use_lj or biteq(glj[:B * d].view(B, d), want_lj), (B, use_z, use_lj)
