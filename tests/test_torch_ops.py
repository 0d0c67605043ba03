"""The torch.ops.umnn custom ops without a GPU: registration, schemas, fake-tensor shapes (what torch.compile / torch.export
trace with), the ATen backward they fall back to, and the guard on native pointers under torch.jit.trace."""
import subprocess
import sys

import pytest
import torch
from torch._subclasses.fake_tensor import FakeTensorMode
from torch.fx.experimental.symbolic_shapes import DimDynamic, ShapeEnv, StatelessSymbolicContext

import umnn_amd
from umnn_amd import _lib, integral, made, ops
from umnn_amd.nets import IntegrandNN, IntegrandNetwork
from umnn_amd.quadrature import device_tables

SCHEMA_ARGS = {
    "cc_forward": ["x0", "x", "h", "W", "b", "hidden_act", "out_act", "nb_steps", "inv_f"],
    "cc_backward": ["x0", "x", "h", "g", "g_fx", "W", "b", "hidden_act", "out_act", "nb_steps", "need", "inv_f"],
    "flow_block": ["x", "h", "scaling", "W", "b", "hidden_act", "out_act", "nb_steps", "reverse_z", "log_jac_in"],
    "flow_block_backward": ["x", "h", "scaling", "fx", "gz", "glj", "W", "b", "hidden_act", "out_act", "nb_steps", "reverse_z",
                            "need"],
    "flow_ll": ["z", "log_jac"],
    "flow_ll_backward": ["z", "g_ll"],
    "flow_ll_block": ["x", "h", "scaling", "W", "b", "hidden_act", "out_act", "nb_steps", "reverse_z", "first", "last", "ll_in"],
}
N_OUT = {"cc_forward": 2, "cc_backward": 4, "flow_block": 3, "flow_block_backward": 3, "flow_ll": 1, "flow_ll_backward": 2,
         "flow_ll_block": 2}


@pytest.mark.parametrize("name", sorted(SCHEMA_ARGS))
def test_op_is_registered_with_its_schema(name):
    assert name in ops.OPS
    schema = getattr(torch.ops.umnn, name).default._schema
    assert [a.name for a in schema.arguments] == SCHEMA_ARGS[name]
    assert len(schema.returns) == N_OUT[name]
    assert not any(a.alias_info is not None and a.alias_info.is_write for a in schema.arguments), "no op writes an input"


def _net(E, hidden, device="cuda"):
    sizes = [1 + E] + list(hidden) + [1]
    W = [torch.empty(o, i, device=device) for i, o in zip(sizes, sizes[1:])]
    b = [torch.empty(o, device=device) for o in sizes[1:]]
    return W, b


SHAPES = [(1, 1, 2, 1), (64, 2, 10, 20), (300, 6, 30, 50), (7, 784, 30, 100)]


@pytest.mark.parametrize("B,d,E,n", SHAPES)
@pytest.mark.parametrize("h_dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("with_x0", [False, True])
def test_fake_shapes(B, d, E, n, h_dtype, with_x0):
    with FakeTensorMode():
        x = torch.empty(B, d, device="cuda")
        h = torch.empty(B, E * d, device="cuda", dtype=h_dtype)
        x0 = torch.empty(B, d, device="cuda") if with_x0 else None
        s = torch.empty(d, device="cuda")
        W, b = _net(E, [50, 50, 50])
        n_params = sum(t.numel() for t in W + b)
        F, fx = torch.ops.umnn.cc_forward(x0, x, h, W, b, 0, 0, n, False)
        assert F.shape == fx.shape == (B, d) and F.dtype == fx.dtype == torch.float32 and F.device.type == "cuda"
        dx0, dx, dh, dth = torch.ops.umnn.cc_backward(x0, x, h, F, fx, W, b, 0, 0, n, [True, True, True, True], False)
        assert dx0.shape == ((B, d) if with_x0 else (0,))
        assert dx.shape == (B, d) and dx.dtype == torch.float32
        assert dh.shape == (B, E * d) and dh.dtype == h_dtype
        assert dth.shape == (n_params,) and dth.dtype == torch.float32
        _, dx, dh, dth = torch.ops.umnn.cc_backward(x0, x, h, F, None, W, b, 0, 0, n, [False, True, False, False], False)
        assert dx.shape == (B, d) and dh.numel() == 0 and dth.numel() == 0
        z, lj, fx = torch.ops.umnn.flow_block(x, h, s, W, b, 0, 0, n, True, x0)
        assert z.shape == lj.shape == fx.shape == (B, d) and z.dtype == lj.dtype == torch.float32
        dx, dh, dth = torch.ops.umnn.flow_block_backward(x, h, s, fx, z, lj, W, b, 0, 0, n, True, [True, True, True])
        assert dx.shape == (B, d) and dh.shape == (B, E * d) and dh.dtype == h_dtype and dth.shape == (n_params,)
        ll = torch.ops.umnn.flow_ll(z, lj)
        assert ll.shape == (B,) and ll.dtype == torch.float32
        gz, glj = torch.ops.umnn.flow_ll_backward(z, ll)
        assert gz.shape == glj.shape == (B, d)
        if h_dtype == torch.float32:                # (the one-pass entry point is fp32-only: see the refusals below)
            z, ll = torch.ops.umnn.flow_ll_block(x, h, s, W, b, 0, 0, n, False, True, False, None)
            z, ll = torch.ops.umnn.flow_ll_block(z, h, s, W, b, 0, 0, n, False, False, True, ll)
            assert z.shape == (B, d) and ll.shape == (B,) and ll.dtype == torch.float32


def _refusals():
    """(op call, expected message) pairs: inputs the kernels would read or write out of bounds, or on another device."""
    B, d, E, n = 16, 3, 4, 10
    x, h = torch.empty(B, d, device="cuda"), torch.empty(B, E * d, device="cuda")
    h16, s = h.to(torch.bfloat16), torch.empty(d, device="cuda")
    W, b = _net(E, [20, 20])
    Wc = [w.to("cpu") for w in W]
    z, ll = torch.empty(B, d, device="cuda"), torch.empty(B, device="cuda")
    u = torch.ops.umnn
    return [
        (lambda: u.flow_ll_block(x, h16, s, W, b, 0, 0, n, False, True, True, None), "flow_ll_block: h has dtype torch.bfloat16"),
        (lambda: u.flow_ll_block(x, h, s, W, b, 0, 0, n, False, False, True, ll[:B - 1]), r"flow_ll_block: ll_in has shape \(15,\)"),
        (lambda: u.flow_ll_block(x, h, s, W, b, 0, 0, n, False, False, True, None), "ll_in must be given exactly when first is False"),
        (lambda: u.flow_ll_block(x, h, s.double(), W, b, 0, 0, n, False, True, True, None), "scaling has dtype torch.float64"),
        (lambda: u.cc_forward(None, x, h, Wc, b, 0, 0, n, False), r"cc_forward: W\[0\] is on cpu"),
        (lambda: u.cc_forward(None, x.cpu(), h.cpu(), Wc, [t.cpu() for t in b], 0, 0, n, False), "x is on cpu"),
        (lambda: u.cc_forward(None, x, h[:, :-1], W, b, 0, 0, n, False), r"cc_forward: h has shape"),
        (lambda: u.cc_forward(None, x, h, [w.double() for w in W], b, 0, 0, n, False), "integrand weights must be fp32"),
        (lambda: u.cc_forward(None, x, h, W[:1], b[:1], 0, 0, n, False), "the integrand needs 2 to 8 layers"),
        (lambda: u.cc_forward(None, x, h, W, b, 5, 0, n, False), "unknown hidden_act 5"),
        (lambda: u.cc_backward(None, x, h, z[:, :2], None, W, b, 0, 0, n, [False, True, True, True], False), "g has shape"),
        (lambda: u.cc_backward(z[:8], x, h, z, None, W, b, 0, 0, n, [True, True, True, True], False), "x0 has shape"),
        (lambda: u.flow_block(x, h, s[:2], W, b, 0, 0, n, False, None), "flow_block: scaling has shape"),
        (lambda: u.flow_block(x, h, s, W, b, 0, 0, n, False, ll), "log_jac_in has 1 dimensions"),
        (lambda: u.flow_block_backward(x, h, s, z, z[:8], z, W, b, 0, 0, n, False, [True, True, True]), "gz has shape"),
        (lambda: u.flow_block_backward(x, h, s, z.bfloat16(), z, z, W, b, 0, 0, n, False, [True, True, True]), "fx has dtype"),
        (lambda: u.flow_ll(z.bfloat16(), z), "flow_ll: z has dtype torch.bfloat16"),
        (lambda: u.flow_ll(z, z[:8]), "flow_ll: log_jac has shape"),
        (lambda: u.flow_ll_backward(z, ll[:3]), "flow_ll_backward: g_ll has shape"),
    ]


def test_fakes_refuse_what_the_kernels_cannot_take():
    with FakeTensorMode():
        cases = _refusals()
        for call, msg in cases:
            with pytest.raises(RuntimeError, match=msg):
                call()


def test_flow_block_f_x_is_not_differentiable_and_scaling_must_be_frozen():
    with FakeTensorMode():
        B, d, E = 8, 3, 4
        x = torch.empty(B, d, device="cuda", requires_grad=True)
        h = torch.empty(B, E * d, device="cuda")
        W, b = _net(E, [20, 20])
        W = [w.requires_grad_() for w in W]
        s = torch.empty(d, device="cuda")
        z, lj, fx = torch.ops.umnn.flow_block(x, h, s, W, b, 0, 0, 10, False, None)
        assert z.requires_grad and lj.requires_grad and not fx.requires_grad
        with pytest.raises(RuntimeError, match="no gradient for a trainable scaling"):
            torch.ops.umnn.flow_block(x, h, s.requires_grad_(), W, b, 0, 0, 10, False, None)
        with pytest.raises(RuntimeError, match="differentiable for fp32 x only"):
            torch.ops.umnn.flow_block(x.detach().bfloat16().requires_grad_(), h, s.detach(), W, b, 0, 0, 10, False, None)


def test_fake_shapes_with_a_symbolic_batch():
    mode = FakeTensorMode(shape_env=ShapeEnv())
    ctx = StatelessSymbolicContext(dynamic_sizes=[DimDynamic.DYNAMIC, DimDynamic.STATIC])
    d, E = 6, 30
    x = mode.from_tensor(torch.empty(256, d, device="meta"), symbolic_context=ctx)
    h = mode.from_tensor(torch.empty(256, E * d, device="meta"), symbolic_context=ctx)
    with mode:
        x, h = x.to("cuda"), h.to("cuda")
        W, b = _net(E, [50, 50])
        s = torch.empty(d, device="cuda")
        B = x.shape[0]
        assert isinstance(B, torch.SymInt)
        F, fx = torch.ops.umnn.cc_forward(None, x, h, W, b, 0, 0, 20, False)
        z, ll = torch.ops.umnn.flow_ll_block(x, h, s, W, b, 0, 0, 20, True, True, True, None)
        _, dx, dh, dth = torch.ops.umnn.cc_backward(None, x, h, F, fx, W, b, 0, 0, 20, [False, True, True, True], False)
        z2, lj, _ = torch.ops.umnn.flow_block(x, h, s, W, b, 0, 0, 20, False, None)
        ll2 = torch.ops.umnn.flow_ll(z2, lj)
    for t in (F, fx, z, dx, z2):
        assert t.shape[0] is B or t.shape[0] == B
        assert t.shape[1] == d
    assert isinstance(ll.shape[0], torch.SymInt) and ll.shape[0] == B and ll2.shape[0] == B
    assert dh.shape[0] == B and dh.shape[1] == E * d


@pytest.mark.parametrize("with_x0", [False, True])
def test_the_three_backward_fakes_agree(with_x0):
    """cc_backward, cc_backward_multi and cc_backward_multi_fx share one fake: at B = 4, d = 1, E = 2 (a single-output and a K = 2 net on
    the same hidden layers) every ``need`` mask gives the three the same shapes and dtypes, and empty tensors where need is False."""
    B, E, K = 4, 2, 2
    with FakeTensorMode():
        x, h = torch.empty(B, 1, device="cuda"), torch.empty(B, E, device="cuda", dtype=torch.bfloat16)
        x0 = torch.empty(B, 1, device="cuda") if with_x0 else None
        W, b = _net(E, [20, 20])
        WK, bK = W[:-1] + [torch.empty(K, 20, device="cuda")], b[:-1] + [torch.empty(K, device="cuda")]
        g, gK = torch.empty(B, 1, device="cuda"), torch.empty(B, K, device="cuda")
        n_params = [sum(t.numel() for t in ts) for ts in (W + b, WK + bK)]
        u = torch.ops.umnn
        for mask in range(16):
            need = [bool(mask >> i & 1) for i in range(4)]
            single = u.cc_backward(x0, x, h, g, g, W, b, 0, 0, 10, need, False)
            multi = u.cc_backward_multi(x0, x, h, gK, WK, bK, 0, 0, 10, need, False)
            multi_fx = u.cc_backward_multi_fx(x0, x, h, gK, gK, WK, bK, 0, 0, 10, need, False)
            want = [(B, 1) if need[0] and with_x0 else (0,), (B, 1) if need[1] else (0,), (B, E) if need[2] else (0,)]
            for outs, n in ((single, n_params[0]), (multi, n_params[1]), (multi_fx, n_params[1])):
                assert [tuple(t.shape) for t in outs] == want + [(n,) if need[3] else (0,)], (need, outs)
                assert [t.dtype for t in outs] == [torch.float32, torch.float32, torch.bfloat16, torch.float32]
                assert all(t.device.type == "cuda" for t in outs)


@pytest.mark.parametrize("n_out,d,E", [(3, 1, 3), (1, 3, 2)], ids=["K=3", "d=3"])
def test_pure_mlp_is_the_module_for_every_n_out(n_out, d, E):
    """The one ``ops.pure_mlp`` at B = 5, hidden 7-6: for K = 3 outputs over x [B,1] it is ``IntegrandNN(4, [7, 6], n_out=3)`` on the same
    weights -> [B, 3]; for one output at d = 3, E = 2 it is ``IntegrandNetwork.forward`` -> [B, d].  The same ATen ops in the same
    order (at d = 1 the row gather is the identity), so values are equal bit for bit, and ``torch.func.vjp`` gives the gradients of
    the module's autograd."""
    torch.manual_seed(0)
    B = 5
    net = IntegrandNN(1 + E, [7, 6], n_out=n_out) if n_out > 1 else IntegrandNetwork(d, 1 + E, [7, 6], 1)
    hidden_act = _lib.ACT_RELU if n_out > 1 else _lib.ACT_LEAKY_RELU
    lins = [m for m in net.net if isinstance(m, torch.nn.Linear)]
    f, params = ops.pure_mlp([l.weight for l in lins], [l.bias for l in lins], hidden_act, _lib.OUT_ELU_PLUS_ONE)
    x, h = torch.randn(B, d), torch.randn(B, E * d)
    want = net(x, h)
    assert want.shape == (B, n_out * d)
    got, vjp = torch.func.vjp(f, params, x, h)
    assert torch.equal(got, want) and torch.equal(f(params, x, h), want)
    cot = torch.randn_like(want)
    xr, hr = x.clone().requires_grad_(), h.clone().requires_grad_()
    grads = torch.autograd.grad(net(xr, hr), [xr, hr] + list(net.parameters()), cot)
    g_params, g_x, g_h = vjp(cot)
    for name, a, w in zip(["x", "h"] + [f"parameter {i}" for i in range(len(params))], [g_x, g_h] + list(g_params), grads):
        assert a.shape == w.shape and torch.equal(a, w), name


def test_import_loads_no_library():
    code = ("import sys, torch, umnn_amd\n"
            "from umnn_amd import _lib\n"
            "assert _lib._lib is None, 'libumnn_cc loaded at import'\n"
            "assert all(hasattr(torch.ops.umnn, n) for n in umnn_amd.ops.OPS)\n"
            "maps = open('/proc/self/maps').read() if sys.platform.startswith('linux') else ''\n"
            "assert 'libumnn_cc' not in maps\n"
            "assert not torch.cuda.is_initialized()\n"
            "assert 'torch._dynamo' not in sys.modules, 'import umnn_amd pulled in torch._dynamo'\n"
            "print('ok')\n")
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and out.stdout.strip().endswith("ok"), out.stderr


def _dense_float64_truth(net, x0, x, h, g, gfx, n, inv_f):
    """(dx0, dx, dh, dtheta) of the quadrature from a construction that shares nothing with the implementation: the un-chunked sum
    over all n + 1 nodes of the package's own tables (``device_tables``, widened to float64) as one scalar, differentiated by plain
    ``torch.autograd.grad``; the g_fx term by autograd through f(x; h); the Leibniz terms f(x) g and -f(x0) g."""
    w, s = device_tables(n, x.device)
    w, u = w.double().view(-1), s.double().view(-1) + 1
    hr, xr = h.clone().requires_grad_(True), x.clone().requires_grad_(True)
    params = list(net.parameters())
    total = 0
    for k in range(n + 1):
        f = net(x0 + (x - x0) * u[k] / 2, hr)
        total = total + w[k] * (1 / f if inv_f else f)
    loss = (total * (x - x0) / 2 * g).sum()
    fx = net(xr, hr)
    if gfx is not None:
        loss = loss + (fx * gfx).sum()
    grads = torch.autograd.grad(loss, [hr, xr] + params, allow_unused=True)
    dx = fx.detach() * g + (grads[1] if grads[1] is not None else 0)
    return -net(x0, h).detach() * g, dx, grads[0], torch.cat([p.reshape(-1) for p in grads[2:]])


def _check_aten_backward(hidden, act, with_gfx, inv_f):
    torch.manual_seed(0)
    B, d, E, n = 9, 3, 4, 12
    net = IntegrandNetwork(d, 1 + E, hidden, 1, act_func=act).double()
    x0, x = torch.randn(B, d, dtype=torch.float64), torch.randn(B, d, dtype=torch.float64)
    h, g = torch.randn(B, E * d, dtype=torch.float64), torch.randn(B, d, dtype=torch.float64)
    gfx = torch.randn(B, d, dtype=torch.float64) if with_gfx else None
    want = _dense_float64_truth(net, x0, x, h, g, gfx, n, inv_f)
    lins = [m for m in net.net if isinstance(m, torch.nn.Linear)]
    tensors = ops.pure_mlp([l.weight for l in lins], [l.bias for l in lins], 0, 0 if act == "ELU" else 1)
    for adapter, integrand in (("module", net), ("W[] / b[]", tensors)):
        got = integral.aten_vjp(integrand, x0, x, h, g, gfx, n, inv_f)
        for name, a, w in zip(("dx0", "dx", "dh", "dtheta"), got, want):
            torch.testing.assert_close(a, w.view(a.shape), rtol=1e-10, atol=1e-12, msg=lambda m: f"{adapter} adapter, {name}: {m}")
    if not with_gfx:        # (the reference-shaped return of integrate(compute_grad=True))
        dtheta, dh = integral.aten_backward(net, x0, x, h, g, n, inv_f)
        torch.testing.assert_close(dtheta, want[3], rtol=1e-10, atol=1e-12)
        torch.testing.assert_close(dh, want[2], rtol=1e-10, atol=1e-12)


@pytest.mark.parametrize("hidden,act", [([12, 12], "ELU"), ([10, 20, 10], "Sigmoid")])
@pytest.mark.parametrize("with_gfx", [False, True])
def test_op_aten_backward_matches_the_module_chain(hidden, act, with_gfx):
    """The one ATen quadrature backward (``integral.aten_vjp``: what cc_backward runs for nets the HIP backward turns away, and
    what the eager operators run off the GPU) through both of its adapters -- the module and the ops' W[] / b[] -- against the
    dense float64 quadrature differentiated by plain autograd."""
    _check_aten_backward(hidden, act, with_gfx, False)


@pytest.mark.parametrize("hidden,act", [([12, 12], "ELU"), ([10, 20, 10], "Sigmoid")])
def test_aten_backward_of_an_inverse_integrand_matches_dense_float64(hidden, act):
    """The same for ``inv_f`` (the integral of 1/f; no operator with an f_x output has it, so no g_fx)."""
    _check_aten_backward(hidden, act, False, True)


def test_native_pointers_refuse_jit_trace():
    t = torch.randn(4, 3)

    def via_integral(x):
        integral._ptr(x)
        return x * 2

    def via_made(x):
        made._ptr(x)
        return x * 2

    for fn, name in ((via_integral, "via_integral"), (via_made, "via_made")):
        with pytest.raises(RuntimeError, match=f"{name}\\(\\) passed a tensor to a native call while torch.jit.trace"):
            torch.jit.trace(fn, t)
        assert fn(t).shape == t.shape            # eager: untouched


def test_graph_mode_predicate():
    assert not integral._graph_mode()
    seen = []

    def f(x):
        seen.append(integral._graph_mode())
        return x + 1

    torch.jit.trace(f, torch.randn(2), check_trace=False)
    torch.compile(f, backend="eager", fullgraph=True)(torch.randn(3))
    assert seen == [True, True]


def test_invert_refuses_jit_trace():
    flow = umnn_amd.UMNNMAFFlow(nb_flow=1, nb_in=2, hidden_derivative=[8, 8], hidden_embedding=[8, 8], embedding_s=2,
                                nb_steps=5)
    with pytest.raises(RuntimeError, match="invert cannot be traced"):
        torch.jit.trace(lambda z: flow.invert(z, 2), torch.randn(3, 2))
