"""torch.compile, torch.export and torch.jit.trace of the package's models on the GPU, through the torch.ops.umnn ops: the
graphs keep the HIP kernels and compute what eager computes."""
import warnings

import numpy as np
import pytest
import torch
import torch._dynamo

import umnn_amd
from umnn_amd import integral, ops
from umnn_amd.nets import mlp_spec
from oracle import cc_oracle as O

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")


@pytest.fixture(autouse=True)
def _fresh():
    torch._dynamo.reset()
    old = umnn_amd.get_forward_precision(), umnn_amd.get_backward_precision(), umnn_amd.get_made_fast_path()
    yield
    torch._dynamo.reset()
    umnn_amd.set_forward_precision(old[0])
    umnn_amd.set_backward_precision(old[1])
    umnn_amd.set_made_fast_path(old[2])


def _flow(d, nb_flow, hidden, E, n, cond_in=0, hidden_emb=(64, 64), seed=0):
    torch.manual_seed(seed)
    f = umnn_amd.UMNNMAFFlow(nb_flow=nb_flow, nb_in=d, hidden_derivative=list(hidden), hidden_embedding=list(hidden_emb),
                             embedding_s=E, nb_steps=n, solver="CCParallel", cond_in=cond_in)
    with torch.no_grad():
        for i in range(nb_flow):
            for m in f.nets[i].net.parallel_nets.net:
                if isinstance(m, torch.nn.Linear):
                    m.weight.mul_(1.5)
    return f.to(DEV)


POWER = dict(d=6, nb_flow=2, hidden=[50] * 4, E=30, n=20)
TOY = dict(d=2, nb_flow=1, hidden=[100] * 4, E=10, n=20)


def _oracle_ll(flow, x):
    sd = {k: v.detach().cpu().numpy() for k, v in flow.state_dict().items()}

    def seq(prefix):
        idx = sorted({int(k[len(prefix):].split(".")[0]) for k in sd if k.startswith(prefix) and k.endswith(".weight")})
        return ([sd[f"{prefix}{j}.weight"] for j in idx], [sd[f"{prefix}{j}.bias"] for j in idx],
                [sd.get(f"{prefix}{j}.mask") for j in idx])
    blocks = []
    for i in range(len(flow.nets)):
        mW, mb, mm = seq(f"Flow{i}.net.made.net.")
        iW, ib, _ = seq(f"Flow{i}.net.parallel_nets.net.")
        blocks.append(O.Block(mW, mb, mm, O.Net(iW, ib, O.LEAKY, O.ELU1), sd[f"Flow{i}.scaling"]))
    return O.flow_compute_ll(blocks, x.cpu().numpy(), flow.nets[0].nb_steps)[0]


def _same(a, b):
    assert a.shape == b.shape and a.dtype == b.dtype
    assert torch.equal(a, b), f"max |diff| {(a.float() - b.float()).abs().max().item()}"


def _net_args(E, hidden, d=3, B=64, seed=1):
    torch.manual_seed(seed)
    net = umnn_amd.IntegrandNetwork(d, 1 + E, hidden, 1).to(DEV)
    W, b, ha, oa = ops.spec_args(mlp_spec(net))
    x, x0 = torch.randn(B, d, device=DEV), torch.randn(B, d, device=DEV) * 0.1
    h = torch.randn(B, E * d, device=DEV)
    return net, W, b, ha, oa, x0, x, h


# ---------------------------------------------------------------------------------------------------------------- 1. opcheck
def test_opcheck_every_op():
    net, W, b, ha, oa, x0, x, h = _net_args(4, [32, 32], B=48)
    W, b = [w.detach() for w in W], [t.detach() for t in b]       # (the backward ops and flow_ll_block have no autograd)
    s = torch.rand(3, device=DEV) * 0.1
    Wg = [w.detach().clone().requires_grad_() for w in W]
    bg = [t.detach().clone().requires_grad_() for t in b]
    xg, hg = x.clone().requires_grad_(), h.clone().requires_grad_()
    g = torch.randn_like(x)
    torch.library.opcheck(torch.ops.umnn.cc_forward.default, (x0, xg, hg, Wg, bg, ha, oa, 16, False))
    torch.library.opcheck(torch.ops.umnn.cc_forward.default, (None, x, h, W, b, ha, oa, 16, False))
    torch.library.opcheck(torch.ops.umnn.cc_backward.default, (x0, x, h, g, g * 0.5, W, b, ha, oa, 16, [True, True, True, True], False))
    torch.library.opcheck(torch.ops.umnn.cc_backward.default, (None, x, h, g, None, W, b, ha, oa, 16, [False, True, False, True], False))
    torch.library.opcheck(torch.ops.umnn.flow_block.default, (xg, hg, s, Wg, bg, ha, oa, 16, True, None))
    z, lj, fx = torch.ops.umnn.flow_block(x, h, s, W, b, ha, oa, 16, True, None)
    torch.library.opcheck(torch.ops.umnn.flow_block_backward.default, (x, h, s, fx, g, g * 0.5, W, b, ha, oa, 16, True, [True, True, True]))
    torch.library.opcheck(torch.ops.umnn.flow_ll.default, (z.clone().requires_grad_(), lj.clone().requires_grad_()))
    torch.library.opcheck(torch.ops.umnn.flow_ll_backward.default, (z, torch.randn(48, device=DEV)))
    torch.library.opcheck(torch.ops.umnn.flow_ll_block.default, (x, h, s, W, b, ha, oa, 16, True, True, False, None))
    torch.library.opcheck(torch.ops.umnn.flow_ll_block.default, (z, h, s, W, b, ha, oa, 16, False, False, True, lj[:, 0].contiguous()))


# ---------------------------------------------------------------------------------------------------------------- 2. op == eager
@pytest.mark.parametrize("precision", ["f16x3", "fp32"])
def test_ops_equal_the_eager_functions_bit_for_bit(precision):
    umnn_amd.set_precision(precision)
    net, W, b, ha, oa, x0, x, h = _net_args(10, [50, 50, 50], B=200)
    spec = mlp_spec(net)
    s = torch.rand(3, device=DEV) * 0.1
    g, gfx = torch.randn_like(x), torch.randn_like(x)
    for xx0 in (None, x0):
        F, fx = torch.ops.umnn.cc_forward(xx0, x, h, W, b, ha, oa, 30, False)
        Fe, fxe, _ = integral.hip_forward(spec, xx0, x, h, 30)
        _same(F, Fe)
        _same(fx, fxe)
        need = [xx0 is not None, True, True, True]
        got = torch.ops.umnn.cc_backward(xx0, x, h, g, gfx, W, b, ha, oa, 30, need, False)
        want = integral.hip_backward(spec, xx0, x, h, g, gfx, 30, tuple(need))
        for a, w, n in zip(got, want, need):
            if n:
                _same(a, w)
    z, lj, fx = torch.ops.umnn.flow_block(x, h, s, W, b, ha, oa, 30, True, None)
    ze, lje, fxe, _ = integral.hip_flow_block(spec, x, h, s, 30, True, None)
    _same(z, ze)
    _same(lj, lje)
    _same(fx, fxe)
    z1, ll = torch.ops.umnn.flow_ll_block(x, h, s, W, b, ha, oa, 30, True, True, False, None)
    z2, ll = torch.ops.umnn.flow_ll_block(z1, h, s, W, b, ha, oa, 30, False, False, True, ll)
    lle, scratch = torch.empty(200, device=DEV), torch.empty_like(x)
    z1e = integral.hip_flow_ll_block(spec, x, h, s, 30, True, True, False, lle, scratch)
    z2e = integral.hip_flow_ll_block(spec, z1e, h, s, 30, False, False, True, lle, scratch)
    _same(z2, z2e)
    _same(ll, lle)
    # flow_block_backward against FlowBlockTransform.backward's own steps (with z_2 recomputed, as in graph mode)
    gz, glj = torch.randn_like(x), torch.randn_like(x)
    dx, dh, dth = torch.ops.umnn.flow_block_backward(x, h, s, fx, gz, glj, W, b, ha, oa, 30, True, [True, True, True])
    gF, gfxe = integral.hip_flow_block_cotangents(gz, glj, fxe, s, True)
    _, dxe, dhe, dthe = integral.hip_backward(spec, None, x, h, gF, gfxe, 30, (False, True, True, True), z2_saved=None)
    dhe.view(200, -1, 3)[:, 0, :].add_(gF)
    _same(dx, dxe)
    _same(dh, dhe)
    _same(dth, dthe)
    # flow_ll / flow_ll_backward against FlowLogLikelihood's launches
    _same(torch.ops.umnn.flow_ll(z, lj), integral.hip_flow_ll(z, lj))
    g_ll = torch.randn(200, device=DEV)
    for a, w in zip(torch.ops.umnn.flow_ll_backward(z, g_ll), integral.hip_flow_ll_backward(z, g_ll, True, True)):
        _same(a, w)
    assert umnn_amd.path_taken() == "hip"


# ---------------------------------------------------------------------------------------------------------------- 3. MonotonicNN
def _mono_grads(m, x, h, fn):
    m.zero_grad()
    xg, hg = x.clone().requires_grad_(), h.clone().requires_grad_()
    y = fn(xg, hg)
    (y * torch.linspace(-1, 1, y.shape[0], device=DEV).view(-1, 1)).sum().backward()
    return [y.detach(), xg.grad, hg.grad] + [p.grad.clone() for p in m.parameters()]


def test_monotonic_nn_compiles_and_matches_eager_bit_for_bit():
    torch.manual_seed(0)
    m = umnn_amd.MonotonicNN(3, [100, 100, 100], nb_steps=50).to(DEV)
    x, h = torch.randn(512, 1, device=DEV), torch.randn(512, 2, device=DEV)
    want = _mono_grads(m, x, h, m)
    cm = torch.compile(m, backend="aot_eager", fullgraph=True)
    got = _mono_grads(m, x, h, cm)
    for a, w in zip(got, want):
        _same(a, w)
    assert umnn_amd.path_taken() == "hip" and umnn_amd.backward_path_taken() == "hip"


# ---------------------------------------------------------------------------------------------------------------- 4. compute_ll inference
def _ll_fn(flow):
    def f(x):
        with torch.no_grad():
            return flow.compute_ll(x)[0]
    return f


@pytest.mark.parametrize("shape,B", [(POWER, 256), (TOY, 500)], ids=["power", "toy"])
def test_compute_ll_inference_compiles(shape, B):
    flow = _flow(**shape)
    x = torch.randn(B, shape["d"], device=DEV)
    umnn_amd.set_precision("fp32")
    want = _ll_fn(flow)(x)
    got = torch.compile(_ll_fn(flow), backend="aot_eager", fullgraph=True)(x)
    _same(got, want)
    torch._dynamo.reset()
    umnn_amd.set_precision("f16x3")
    want = _ll_fn(flow)(x)
    got = torch.compile(_ll_fn(flow), backend="aot_eager", fullgraph=True)(x)
    assert ((got - want).abs() / want.abs().clamp(min=1)).max().item() < 1e-4
    ref = _oracle_ll(flow, x)
    assert float(np.max(np.abs(got.cpu().numpy() - ref) / np.maximum(np.abs(ref), 1.0))) < 1e-4
    torch._dynamo.reset()
    ex = torch._dynamo.explain(_ll_fn(flow))(x)
    assert ex.graph_break_count == 0 and ex.graph_count == 1
    code = ex.graphs[0].code
    assert code.count("umnn.flow_ll_block") == shape["nb_flow"]


# ---------------------------------------------------------------------------------------------------------------- 5. training
def _train_grads(flow, x, fn):
    flow.zero_grad()
    loss = fn(x)
    loss.backward()
    return [loss.detach()] + [p.grad.clone() for p in flow.parameters() if p.grad is not None]


def _loss_fn(flow, context=None):
    def f(x):
        return -flow.compute_ll(x, context)[0].mean()
    return f


@pytest.mark.parametrize("shape,B", [(POWER, 256), (dict(d=784, nb_flow=1, hidden=[100, 50, 50, 50, 50], E=10, n=20), 32)],
                         ids=["power", "mnist_front"])
def test_training_step_compiles(shape, B):
    umnn_amd.set_precision("fp32")
    flow = _flow(**shape)
    x = torch.randn(B, shape["d"], device=DEV) * 0.5
    want = _train_grads(flow, x, _loss_fn(flow))
    got = _train_grads(flow, x, torch.compile(_loss_fn(flow), backend="aot_eager", fullgraph=True))
    assert len(got) == len(want)
    for a, w in zip(got, want):
        assert (a - w).abs().max().item() <= 1e-5 * max(w.abs().max().item(), 1e-30)
    assert umnn_amd.backward_path_taken() == "hip"


def test_training_step_compiles_with_the_aten_backward():
    """A deep wide integrand (five unequal hidden layers above 63 units, as in test_gpu_round3.py): the HIP backward has no
    shape-exact kernel, so cc_backward runs the ATen backward (integral.aten_vjp on the ops' W[] / b[]) inside the compiled
    graph, against eager's, on the module."""
    flow = _flow(d=3, nb_flow=2, hidden=[100, 72, 80, 96, 70], E=4, n=10)
    x = torch.randn(32, 3, device=DEV) * 0.5
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")             # (the once-per-process announcement of the ATen backward)
        want = _train_grads(flow, x, _loss_fn(flow))
    assert umnn_amd.backward_path_taken() == "aten"
    integral._last_backward["path"] = None
    got = _train_grads(flow, x, torch.compile(_loss_fn(flow), backend="aot_eager", fullgraph=True))
    assert umnn_amd.backward_path_taken() == "aten"
    assert len(got) == len(want)
    for a, w in zip(got, want):
        assert (a - w).abs().max().item() <= 1e-5 * max(w.abs().max().item(), 1e-30)


def test_compute_log_jac_and_integrate_compile():
    umnn_amd.set_precision("fp32")
    flow = _flow(**POWER)
    blk = flow.nets[0]
    x = torch.randn(128, 6, device=DEV)

    def lj(x):
        with torch.no_grad():
            return blk.compute_log_jac(x)
    _same(torch.compile(lj, backend="aot_eager", fullgraph=True)(x), lj(x))
    integrand = blk.net.parallel_nets
    h = torch.randn(128, 30 * 6, device=DEV)
    x0 = torch.zeros_like(x)

    def fwd(x, h):
        return umnn_amd.integrate(x0, 20, x / 20, integrand, h)

    def grads(x, h):
        return umnn_amd.integral.integrate(x0, 20, x / 20, integrand, h, compute_grad=True, x_tot=torch.ones_like(x))
    torch._dynamo.reset()
    with torch.no_grad():
        _same(torch.compile(fwd, backend="aot_eager", fullgraph=True)(x, h), fwd(x, h))
    torch._dynamo.reset()
    for a, w in zip(torch.compile(grads, backend="aot_eager", fullgraph=True)(x, h), grads(x, h)):
        _same(a, w.view(a.shape))


# ---------------------------------------------------------------------------------------------------------------- 6. recompiles
def test_dynamic_batch_and_step_count_recompile_correctly():
    umnn_amd.set_precision("fp32")
    flow = _flow(**POWER)
    cfn = torch.compile(_ll_fn(flow), backend="aot_eager", fullgraph=True, dynamic=True)
    for B, n in ((256, 20), (300, 20), (300, 35), (128, 7)):
        flow.set_steps_nb(n)
        x = torch.randn(B, 6, device=DEV)
        _same(cfn(x), _ll_fn(flow)(x))


# ---------------------------------------------------------------------------------------------------------------- 7. jit.trace
def test_jit_trace_replays_save_load_and_invert_raises(tmp_path):
    umnn_amd.set_precision("fp32")
    flow = _flow(**POWER)
    flow.eval()
    for p in flow.parameters():
        p.requires_grad_(False)
    x1, x2 = torch.randn(256, 6, device=DEV), torch.randn(256, 6, device=DEV)
    tr = torch.jit.trace(lambda x: flow.compute_ll(x)[0], x1, check_trace=False)
    assert "umnn::flow_ll_block" in tr.graph.str()
    _same(tr(x2), _ll_fn(flow)(x2))
    path = str(tmp_path / "ll.pt")
    torch.jit.save(tr, path)
    loaded = torch.jit.load(path, map_location=DEV)
    _same(loaded(x2), _ll_fn(flow)(x2))
    with pytest.raises(RuntimeError, match="invert cannot be traced"):
        torch.jit.trace(lambda z: flow.invert(z, 3), x1, check_trace=False)


# ---------------------------------------------------------------------------------------------------------------- 8. export
class _LL(torch.nn.Module):
    def __init__(self, flow):
        super().__init__()
        self.flow = flow

    def forward(self, x):
        return self.flow.compute_ll(x)[0]


def test_export_with_a_dynamic_batch():
    umnn_amd.set_precision("fp32")
    torch.manual_seed(0)
    m = umnn_amd.MonotonicNN(3, [50, 50, 50], nb_steps=30).to(DEV)
    batch = torch.export.Dim("batch", min=2, max=4096)
    x, h = torch.randn(64, 1, device=DEV), torch.randn(64, 2, device=DEV)
    ep = torch.export.export(m, (x, h), dynamic_shapes=({0: batch}, {0: batch}))
    assert "torch.ops.umnn.cc_forward" in ep.graph_module.print_readable(print_output=False)
    for B in (64, 300):
        x, h = torch.randn(B, 1, device=DEV), torch.randn(B, 2, device=DEV)
        with torch.no_grad():
            _same(ep.module()(x, h), m(x, h))
    flow = _flow(**POWER)
    for p in flow.parameters():
        p.requires_grad_(False)
    x = torch.randn(256, 6, device=DEV)
    ep = torch.export.export(_LL(flow), (x,), dynamic_shapes=({0: batch},))
    assert "torch.ops.umnn.flow_ll_block" in ep.graph_module.print_readable(print_output=False)
    for B in (256, 300):
        x = torch.randn(B, 6, device=DEV)
        _same(ep.module()(x), _ll_fn(flow)(x))


# ---------------------------------------------------------------------------------------------------------------- 9. conditional, bf16 embedding
def test_conditional_flow_with_bf16_embedding_compiles():
    d, cond = 16, 8
    flow = _flow(d=d, nb_flow=2, hidden=[100] * 4, E=20, n=20, cond_in=cond, hidden_emb=(128, 128))
    flow.set_embedding_dtype(torch.bfloat16)
    x, c = torch.randn(256, d, device=DEV), torch.randn(256, cond, device=DEV)

    def ll(x, c):
        with torch.no_grad():
            return flow.compute_ll(x, c)[0]
    want = ll(x, c)
    got = torch.compile(ll, backend="aot_eager", fullgraph=True)(x, c)
    assert ((got - want).abs() / want.abs().clamp(min=1)).max().item() < 2e-2
    torch._dynamo.reset()
    want = _train_grads(flow, x, _loss_fn(flow, c))
    got = _train_grads(flow, x, torch.compile(_loss_fn(flow, c), backend="aot_eager", fullgraph=True))
    for a, w in zip(got, want):
        assert (a - w).abs().max().item() <= 5e-2 * max(w.abs().max().item(), 1e-30)


# ---------------------------------------------------------------------------------------------------------------- 10. eager stays eager
def test_eager_dispatches_no_umnn_op():
    from torch.utils._python_dispatch import TorchDispatchMode

    class Rec(TorchDispatchMode):
        def __init__(self):
            super().__init__()
            self.names = set()

        def __torch_dispatch__(self, func, types, args=(), kwargs=None):
            self.names.add(str(func))
            return func(*args, **(kwargs or {}))

    flow = _flow(**POWER)
    x = torch.randn(256, 6, device=DEV)
    with Rec() as rec:
        _ll_fn(flow)(x)
        _loss_fn(flow)(x).backward()
    assert rec.names and not any("umnn" in n for n in rec.names), sorted(n for n in rec.names if "umnn" in n)


# ---------------------------------------------------------------------------------------------------------------- 11. Inductor
def test_inductor_monotonic_and_compute_ll():
    pytest.importorskip("triton")
    import torch._inductor.config as icfg
    old = icfg.compile_threads
    icfg.compile_threads = 4
    try:
        torch.manual_seed(0)
        m = umnn_amd.MonotonicNN(3, [100, 100, 100], nb_steps=50).to(DEV)
        x, h = torch.randn(512, 1, device=DEV), torch.randn(512, 2, device=DEV)
        want = _mono_grads(m, x, h, m)
        got = _mono_grads(m, x, h, torch.compile(m, fullgraph=True))
        for a, w in zip(got, want):
            assert (a - w).abs().max().item() <= 1e-4 * max(w.abs().max().item(), 1.0)
        flow = _flow(**POWER)
        x = torch.randn(256, 6, device=DEV)
        want = _ll_fn(flow)(x)
        got = torch.compile(_ll_fn(flow), fullgraph=True)(x)
        assert ((got - want).abs() / want.abs().clamp(min=1)).max().item() < 1e-4
    finally:
        icfg.compile_threads = old
