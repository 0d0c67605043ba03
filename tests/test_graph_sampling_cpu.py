"""Graph-mode sampling without a GPU: the ``umnn::cc_solve_block`` op (schema, fake implementation, refusals), what is importable,
and the sampling calls whose behaviour does not change (torch.jit.trace raises, host tensors take the eager call)."""
import pytest
import torch
from torch._subclasses.fake_tensor import FakeTensorMode
from torch.fx.experimental.symbolic_shapes import DimDynamic, ShapeEnv, StatelessSymbolicContext

import umnn_amd
from umnn_amd import ops


def _net(E, hidden, device="cuda"):
    sizes = [1 + E] + list(hidden) + [1]
    W = [torch.empty(o, i, device=device) for i, o in zip(sizes, sizes[1:])]
    b = [torch.empty(o, device=device) for o in sizes[1:]]
    return W, b


def test_op_is_registered_with_its_schema():
    assert "cc_solve_block" in ops.OPS and hasattr(torch.ops.umnn, "cc_solve_block")
    schema = torch.ops.umnn.cc_solve_block.default._schema
    assert [a.name for a in schema.arguments] == ["t", "h", "x_init", "W", "b", "hidden_act", "out_act", "nb_steps", "lo", "hi", "tol",
                                                  "max_iter"]
    assert len(schema.returns) == 3
    assert not any(a.alias_info is not None and a.alias_info.is_write for a in schema.arguments), "the op writes no input"
    assert "cc_solve_block" in ops.__doc__


def test_public_names_without_a_gpu():
    assert umnn_amd.GraphedSampler is umnn_amd.graphs.GraphedSampler and "GraphedSampler" in umnn_amd.__all__
    assert callable(umnn_amd.ops.cc_solve_block)


@pytest.mark.parametrize("B,d,E", [(1, 1, 2), (37, 5, 4), (7, 784, 30)])
@pytest.mark.parametrize("h_dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("warm", [False, True])
def test_fake_shapes(B, d, E, h_dtype, warm):
    with FakeTensorMode():
        t = torch.empty(B, d, device="cuda")
        h = torch.empty(B, E * d, device="cuda", dtype=h_dtype)
        W, b = _net(E, [50, 50])
        x, fx, status = torch.ops.umnn.cc_solve_block(t, h, torch.empty(B, d, device="cuda") if warm else None, W, b, 0, 0, 12, -50., 50.,
                                                      1e-6, 64)
        assert x.shape == fx.shape == status.shape == (B, d) and x.device.type == "cuda"
        assert x.dtype == fx.dtype == torch.float32 and status.dtype == torch.int32


def test_fake_shapes_with_a_symbolic_batch():
    mode = FakeTensorMode(shape_env=ShapeEnv())
    ctx = StatelessSymbolicContext(dynamic_sizes=[DimDynamic.DYNAMIC, DimDynamic.STATIC])
    d, E = 6, 30
    t = mode.from_tensor(torch.empty(256, d, device="meta"), symbolic_context=ctx)
    h = mode.from_tensor(torch.empty(256, E * d, device="meta"), symbolic_context=ctx)
    with mode:
        t, h = t.to("cuda"), h.to("cuda")
        W, b = _net(E, [50, 50])
        B = t.shape[0]
        assert isinstance(B, torch.SymInt)
        x, fx, status = torch.ops.umnn.cc_solve_block(t, h, None, W, b, 0, 0, 20, -50., 50., 1e-6, 64)
        x2, _, _ = torch.ops.umnn.cc_solve_block(t, h, x, W, b, 0, 0, 20, -50., 50., 1e-6, 64)
    for out in (x, fx, status, x2):
        assert isinstance(out.shape[0], torch.SymInt) and out.shape[0] == B and out.shape[1] == d
    assert status.dtype == torch.int32


def test_fake_refuses_what_the_kernel_cannot_take():
    with FakeTensorMode():
        B, d, E, n = 16, 3, 4, 10
        t, h = torch.empty(B, d, device="cuda"), torch.empty(B, E * d, device="cuda")
        W, b = _net(E, [20, 20])
        u = torch.ops.umnn.cc_solve_block
        cases = [
            (lambda: u(t.cpu(), h.cpu(), None, [w.cpu() for w in W], [v.cpu() for v in b], 0, 0, n, -50., 50., 1e-6, 64), "t|x is on cpu"),
            (lambda: u(t, h.cpu(), None, W, b, 0, 0, n, -50., 50., 1e-6, 64), "cc_solve_block: h is on cpu"),
            (lambda: u(t, h, None, [w.cpu() for w in W], b, 0, 0, n, -50., 50., 1e-6, 64), r"cc_solve_block: W\[0\] is on cpu"),
            (lambda: u(t, h, t.cpu(), W, b, 0, 0, n, -50., 50., 1e-6, 64), "cc_solve_block: x_init is on cpu"),
            (lambda: u(t.double(), h, None, W, b, 0, 0, n, -50., 50., 1e-6, 64), "cc_solve_block: x has dtype torch.float64"),
            (lambda: u(t.bfloat16(), h, None, W, b, 0, 0, n, -50., 50., 1e-6, 64), "cc_solve_block: x has dtype torch.bfloat16"),
            (lambda: u(t, h.double(), None, W, b, 0, 0, n, -50., 50., 1e-6, 64), "cc_solve_block: h has dtype torch.float64"),
            (lambda: u(t, h, t.bfloat16(), W, b, 0, 0, n, -50., 50., 1e-6, 64), "cc_solve_block: x_init has dtype torch.bfloat16"),
            (lambda: u(t, h, t[:8], W, b, 0, 0, n, -50., 50., 1e-6, 64), r"cc_solve_block: x_init has shape \(8, 3\)"),
            (lambda: u(t, h, t[:, :2], W, b, 0, 0, n, -50., 50., 1e-6, 64), r"cc_solve_block: x_init has shape \(16, 2\)"),
            (lambda: u(t, h, t[:, 0], W, b, 0, 0, n, -50., 50., 1e-6, 64), "cc_solve_block: x_init has 1 dimensions"),
            (lambda: u(t, h[:, :-1], None, W, b, 0, 0, n, -50., 50., 1e-6, 64), "cc_solve_block: h has shape"),
            (lambda: u(t, h, None, W, b, 0, 0, n, 3., 3., 1e-6, 64), "cc_solve_block: empty bracket"),
            (lambda: u(t, h, None, W, b, 0, 0, n, 5., -5., 1e-6, 64), "cc_solve_block: empty bracket"),
            (lambda: u(t, h, None, W, b, 0, 0, n, -50., 50., 1e-6, 0), "cc_solve_block: max_iter is 0"),
            (lambda: u(t, h, None, W, b, 0, 0, n, -50., 50., 1e-6, umnn_amd.SOLVE_EVALS_MASK + 1), "cc_solve_block: max_iter is"),
            (lambda: u(t, h, None, W, b, 0, 0, 0, -50., 50., 1e-6, 64), "cc_solve_block: nb_steps is 0"),
            (lambda: u(t, h, None, W, b, 0, 0, n, -50., 50., -1., 64), "cc_solve_block: tol is -1"),
            (lambda: u(t, h, None, W[:1], b[:1], 0, 0, n, -50., 50., 1e-6, 64), "the integrand needs 2 to 8 layers"),
        ]
        for call, msg in cases:
            with pytest.raises(RuntimeError, match=msg):
                call()


def test_the_op_does_not_detach_silently():
    """No autograd formula: the op's outputs join the autograd graph of an input that requires grad -- never a silent detach; the
    backward through that node raises (run where there is a device: tests/test_gpu_graph_sampling.py)."""
    with FakeTensorMode():
        B, d, E = 8, 3, 4
        t = torch.empty(B, d, device="cuda", requires_grad=True)
        h = torch.empty(B, E * d, device="cuda")
        W, b = _net(E, [20, 20])
        x, _, _ = torch.ops.umnn.cc_solve_block(t, h, None, W, b, 0, 0, 10, -50., 50., 1e-6, 64)
        assert x.requires_grad and x.grad_fn is not None


def test_graphed_sampler_checks_its_options_before_it_touches_a_device():
    flow = umnn_amd.UMNNMAFFlow(nb_flow=1, nb_in=2, hidden_derivative=[8, 8], hidden_embedding=[8, 8], embedding_s=2, nb_steps=5)
    with pytest.raises(ValueError, match="sweep_tol=0 and max_sweeps"):
        umnn_amd.GraphedSampler(flow, 4, method="jacobi")
    with pytest.raises(ValueError, match="sweep_tol=0 and max_sweeps"):
        umnn_amd.GraphedSampler(flow, 4, method="jacobi", sweep_tol=0)
    with pytest.raises(ValueError, match="sweep_tol=0 and max_sweeps"):
        umnn_amd.GraphedSampler(flow, 4, method="jacobi", max_sweeps=2)
    with pytest.raises(ValueError, match="'newton' or 'jacobi'"):
        umnn_amd.GraphedSampler(flow, 4, method="bracket")
    with pytest.raises(ValueError, match="no option"):
        umnn_amd.GraphedSampler(flow, 4, method="newton", max_sweeps=2)


def _small_flow():
    torch.manual_seed(0)
    return umnn_amd.UMNNMAFFlow(nb_flow=2, nb_in=3, hidden_derivative=[8, 8], hidden_embedding=[8, 8], embedding_s=2, nb_steps=5).eval()


def test_invert_still_refuses_jit_trace():
    flow = _small_flow()
    for kw in (dict(), dict(method="newton"), dict(method="jacobi", sweep_tol=0, max_sweeps=2)):
        with pytest.raises(RuntimeError, match="invert cannot be traced by torch.jit.trace"):
            torch.jit.trace(lambda z: flow.invert(z, **kw), torch.randn(3, 3))


@pytest.mark.parametrize("kw", [dict(iter=3), dict(method="newton"), dict(method="jacobi", sweep_tol=0, max_sweeps=3)],
                         ids=["bracket", "newton", "jacobi"])
def test_compiled_invert_on_host_tensors_is_the_eager_call(kw):
    """Off the HIP path nothing is recorded: a compiled caller gets the eager result bit for bit, and no ``umnn`` op is called."""
    import warnings
    flow = _small_flow()
    z = torch.randn(5, 3, generator=torch.Generator().manual_seed(1))
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")             # (the once-per-process announcement of the ATen path)
        with torch.no_grad():
            want = flow.invert(z, **kw)
            torch._dynamo.reset()
            got = torch.compile(lambda z: flow.invert(z, **kw), backend="eager")(z)
            torch._dynamo.reset()
    assert torch.equal(got, want)
