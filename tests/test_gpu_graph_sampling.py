"""Graph-mode sampling on the device: the ``umnn::cc_solve_block`` op, ``invert`` as torch.compile / torch.export record it, and
``GraphedSampler`` (the sampling direction as one hipGraph).

Acceptance of every sampler is the round trip of tests/test_gpu_jacobi.py: x -> z = flow(x) -> sampler -> x_hat with |x_hat - x| within
the flow bound -- the sum over the blocks of TOL / min exp(s) f from the model's float64 copy, TOL = 1e-4 the forward parity tolerance:
derived, not measured, and independent of which conditioner composition produced h -- and flow(x_hat) = z to TOL relative.  The bound
is re-stated here (``_flow_bound``).  Flows, inputs and bounds are computed once per flow and never modified; the tests that move
weights work on a copy."""
import copy
import types

import numpy as np
import pytest
import torch
import torch._dynamo

import umnn_amd
from umnn_amd import _lib, integral as I, ops
from umnn_amd.nets import mlp_spec

pytestmark = pytest.mark.gpu
TOL = 1e-4
SOLVE_TOL = 1e-6            # invert's default ``tol`` and ``sweep_tol``
MODES = ["f16x3", "bf16x3", "bf16x6", "fp32"]
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


def _launches():
    return _lib.lib().umnn_launch_count()


def _rel_err(a, b):
    a, b = a.detach().cpu().double(), b.detach().cpu().double()
    return float(((a - b).abs() / b.abs().clamp(min=1.)).max())


def _same(a, b):
    assert a.shape == b.shape and a.dtype == b.dtype
    assert torch.equal(a, b), f"max |diff| {(a.float() - b.float()).abs().max().item()}"


# ---------------------------------------------------------------------------------------------------------------- the flows
def _flow_bound(m, x, context, tol=TOL):
    """sum over blocks of tol / min exp(s) f, from the model's own log_jac pieces in float64 on the CPU."""
    m64 = copy.deepcopy(m).to("cpu").double()
    umnn_amd.invalidate_caches(m64)
    xi = x.detach().cpu().double()
    ctx = None if context is None else context.detach().cpu().double()
    total = 0.
    with torch.no_grad():
        for blk in m64.nets:
            z, lj = blk._transform(xi, ctx, want_jac=True)
            total += tol / float(torch.exp(lj.min()))
            xi = torch.flip(z, [1])
    return total


def _make_flow(d, hid, E, n, nb_flow, seed, cond_in=0, made_gain=1.):
    torch.manual_seed(seed)
    m = umnn_amd.UMNNMAFFlow(nb_flow=nb_flow, nb_in=d, hidden_derivative=list(hid), hidden_embedding=[64, 64], embedding_s=E,
                             nb_steps=n, solver="CCParallel", cond_in=cond_in).to(DEV).eval()
    if made_gain != 1.:
        with torch.no_grad():
            for blk in m.nets:
                for mod in blk.net.made.net:
                    if hasattr(mod, "weight"):
                        mod.weight.mul_(made_gain)
        umnn_amd.invalidate_caches(m)
    for p in m.parameters():
        p.requires_grad_(False)
    return m


# (d, integrand widths, E, n, blocks, B) of tests/test_gpu_jacobi.py's FLOWS and its conditional flow (MADE weights x 3, context of 3)
FLOWS = {"d7": dict(d=7, hid=[50] * 4, E=30, n=50, nb_flow=2, B=33, seed=37),
         "d2": dict(d=2, hid=[100] * 4, E=10, n=50, nb_flow=1, B=64, seed=12),
         "d5": dict(d=5, hid=[100, 50, 50, 50, 50], E=8, n=30, nb_flow=1, B=20, seed=13),
         "cond": dict(d=3, hid=[50] * 4, E=30, n=20, nb_flow=2, B=33, seed=23, cond_in=3, made_gain=3.)}
# the export test's flow (also of that list): d = 3 <= the four sweeps its module asks for, so those are the sequential answer
EXTRA = {"d3": dict(d=3, hid=[40, 33], E=4, n=20, nb_flow=2, B=17, seed=7)}
_CASES = {}


def _case(name):
    if name not in _CASES:
        f = dict(FLOWS[name] if name in FLOWS else EXTRA[name])
        B = f.pop("B")
        m = _make_flow(**f)
        g = torch.Generator().manual_seed(B)
        x = (1.5 * torch.randn(B, f["d"], generator=g)).to(DEV)
        ctx = torch.randn(B, f["cond_in"], generator=g).to(DEV) if f.get("cond_in") else None
        with torch.no_grad():
            z = m(x, context=ctx)
            x_newton = m.invert(z, method="newton", context=ctx)
            # the sweep at which eager jacobi's own test is met; one more than d allowed, where it holds by construction
            _, info = m.invert(z, method="jacobi", context=ctx, max_sweeps=f["d"] + 1, return_info=True)
        _CASES[name] = types.SimpleNamespace(m=m, x=x, ctx=ctx, z=z, d=f["d"], nb_flow=f["nb_flow"], B=B, x_newton=x_newton,
                                             bound=_flow_bound(m, x, ctx), made_layers=3, sweeps=max(info["sweeps"]))
    return _CASES[name]


def _check_round_trip(m, x, ctx, z, bound, x_hat, tag):
    with torch.no_grad():
        z_back = m(x_hat, context=ctx)
    err, rel = float((x_hat - x).abs().max()), _rel_err(z_back, z)
    print(f"{tag}: |x_hat - x| {err:.2e} (bound {bound:.2e}), flow(x_hat) against z {rel:.2e}")
    assert x_hat.shape == x.shape and x_hat.dtype == torch.float32
    assert err <= bound, tag
    assert rel < TOL, tag


def _check_last_move(c, mv, tag):
    """``last_move`` after K >= ``c.sweeps`` sweeps, the count at which eager jacobi met its test (no entry moved by more than
    sweep_tol max(1, |x|); at most d + 1, where every dimension is final by construction).  From that sweep on an entry moves only by
    what two solves to ``tol`` leave undetermined -- each root is pinned to tol / min exp(s) f, the flow bound at tol instead of TOL --
    so last_move <= sweep_tol + 2 bound(tol)."""
    move_bound = SOLVE_TOL + 2 * c.bound * (SOLVE_TOL / TOL)
    print(f"{tag}: last_move {float(mv):.2e} (eager sweeps {c.sweeps}, d = {c.d}, bound {move_bound:.2e})")
    assert mv.dim() == 0 and mv.is_cuda and np.isfinite(float(mv)) and float(mv) <= move_bound, tag


# ---------------------------------------------------------------------------------------------------------------- 1. the op
def _op_case(B, d, E, hid, n, seed=0):
    torch.manual_seed(seed)
    net = umnn_amd.IntegrandNetwork(d, 1 + E, list(hid), 1).to(DEV)
    W, b, ha, oa = ops.spec_args(mlp_spec(net))
    W, b = [w.detach() for w in W], [v.detach() for v in b]
    g = torch.Generator().manual_seed(B + d)
    t = torch.randn(B, d, generator=g).to(DEV)
    h = torch.randn(B, E * d, generator=g).to(DEV)
    x_init = (0.5 * torch.randn(B, d, generator=g)).to(DEV)
    return net, W, b, ha, oa, t, h, x_init, n


def test_opcheck():
    net, W, b, ha, oa, t, h, x_init, n = _op_case(37, 5, 4, [50, 50], 12)
    torch.library.opcheck(torch.ops.umnn.cc_solve_block.default, (t, h, None, W, b, ha, oa, n, -50., 50., 1e-6, 64))
    torch.library.opcheck(torch.ops.umnn.cc_solve_block.default, (t, h, x_init, W, b, ha, oa, n, -50., 50., 1e-6, 64))


@pytest.mark.parametrize("precision", MODES)
@pytest.mark.parametrize("B,d", [(37, 5), (2050, 8)], ids=["split_plan_185_rows", "tile_per_wave_16400_rows"])
def test_op_equals_hip_solve_block_bit_for_bit(B, d, precision):
    """37 x 5 rows: one tile per workgroup; 2050 x 8 = 16 400 rows, above the 16 389 at which tests/test_gpu_solve_coverage.py finds
    one tile per wave.  Cold and warm-started; no input is written."""
    umnn_amd.set_forward_precision(precision)
    net, W, b, ha, oa, t, h, x_init, n = _op_case(B, d, 4, [50, 50], 12)
    spec = mlp_spec(net)
    keep = t.clone(), h.clone(), x_init.clone()
    for start in (None, x_init):
        before = _launches()
        got = torch.ops.umnn.cc_solve_block(t, h, start, W, b, ha, oa, n, -50., 50., 1e-6, 64)
        assert _launches() - before == 1 and umnn_amd.path_taken() == "hip"
        assert _lib.lib().umnn_last_kernel_name().decode().startswith("cc_solve_")
        want = I.hip_solve_block(spec, h, t, n, scaling=None, off_h0=False, x_init=start, lo=-50., hi=50., tol=1e-6, max_iter=64)
        for a, w in zip(got, want):
            _same(a, w)
        assert got[2].dtype == torch.int32 and torch.isfinite(got[0]).all()
        assert all(a.data_ptr() not in (t.data_ptr(), h.data_ptr(), x_init.data_ptr()) for a in got), "fresh outputs"
    for a, k in zip((t, h, x_init), keep):
        _same(a, k)


def test_op_runs_the_host_loop_for_a_net_outside_the_solve_tables():
    """Six hidden layers of 80 units: their two-piece images exceed the LDS the solve kernels accept
    (tests/test_gpu_solve_coverage.py::test_images_beyond_the_lds_run_the_host_loop).  The op then is ``integral.newton_solve`` over
    [B, d] on the forward kernel -- ``integral.host_solve`` bit for bit -- with residuals inside tol max(1, |t|) in that forward."""
    import warnings
    net, W, b, ha, oa, t, h, x_init, n = _op_case(9, 3, 4, [80] * 6, 20)
    spec = mlp_spec(net)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)           # (the fallback is announced once per process)
        for start in (None, x_init):
            got = torch.ops.umnn.cc_solve_block(t, h, start, W, b, ha, oa, n, -50., 50., 1e-6, 64)
            assert umnn_amd.path_taken() == "hip" and not _lib.lib().umnn_last_kernel_name().decode().startswith("cc_solve_")
            want = I.host_solve(spec, h, t, n, -50., 50., 1e-6, 64, x_init=start)
            for a, w in zip(got, want):
                _same(a, w)
            free = (got[2] & (umnn_amd.SOLVE_CLAMPED | umnn_amd.SOLVE_CAPPED | umnn_amd.SOLVE_NONFINITE)) == 0
            F = I.hip_forward(spec, None, got[0], h, n)[0]
            assert bool(free.any()) and bool((((F - t).abs() <= 1e-6 * t.abs().clamp(min=1.)) | ~free).all())


def test_a_gradient_through_the_op_raises():
    net, W, b, ha, oa, t, h, x_init, n = _op_case(9, 3, 4, [50, 50], 12)
    tg = t.clone().requires_grad_()
    x, _, _ = torch.ops.umnn.cc_solve_block(tg, h, None, W, b, ha, oa, n, -50., 50., 1e-6, 64)
    assert x.requires_grad, "never a silent detach"
    with pytest.raises(RuntimeError, match="cc_solve_block"):
        x.sum().backward()


# ---------------------------------------------------------------------------------------------------------------- 2. recorded invert
def _count(code, op):
    """Calls of ``umnn.<op>`` in a graph's code ("umnn.cc_solve" is also the head of "umnn.cc_solve_block")."""
    n = code.count(f"umnn.{op}")
    return n - code.count("umnn.cc_solve_block") if op == "cc_solve" else n


@pytest.mark.parametrize("name", sorted(FLOWS))
def test_compiled_newton_round_trip(name):
    c = _case(name)

    def fn(z):
        return c.m.invert(z, method="newton", context=c.ctx)
    before = _launches()
    x_hat = torch.compile(fn, backend="aot_eager", fullgraph=True)(c.z)
    assert umnn_amd.path_taken() == "hip" and _launches() - before == c.nb_flow * c.d
    _check_round_trip(c.m, c.x, c.ctx, c.z, c.bound, x_hat, f"compiled newton {name}")
    assert float((x_hat - c.x_newton).abs().max()) <= 2 * c.bound
    torch._dynamo.reset()
    ex = torch._dynamo.explain(fn)(c.z)
    assert ex.graph_break_count == 0 and ex.graph_count == 1
    code = ex.graphs[0].code
    assert _count(code, "cc_solve") == c.nb_flow * c.d and _count(code, "cc_solve_block") == 0


@pytest.mark.parametrize("name", sorted(FLOWS))
def test_compiled_jacobi_round_trip(name):
    """``max_sweeps=d``: the sequential answer by construction, so also eager ``invert(method="newton")`` within twice the flow bound
    (each of the two is within one bound of the exact inverse).  ``last_move`` with K >= the eager sweep count (``_check_last_move``)."""
    c = _case(name)

    def fn(z):
        return c.m.invert(z, method="jacobi", context=c.ctx, sweep_tol=0, max_sweeps=c.d, return_info=True)
    before = _launches()
    x_hat, info = torch.compile(fn, backend="aot_eager", fullgraph=True)(c.z)
    assert umnn_amd.path_taken() == "hip" and _launches() - before == c.nb_flow * c.d
    _check_round_trip(c.m, c.x, c.ctx, c.z, c.bound, x_hat, f"compiled jacobi {name}")
    diff = float((x_hat - c.x_newton).abs().max())
    print(f"recorded jacobi against eager newton: {diff:.2e} (2 x bound {2 * c.bound:.2e})")
    assert diff <= 2 * c.bound
    assert info["sweeps"] == [c.d] * c.nb_flow and len(info["status"]) == len(info["last_move"]) == c.nb_flow
    for st, mv in zip(info["status"], info["last_move"]):
        assert st.shape == c.z.shape and st.dtype == torch.int32
        assert not bool((st & (umnn_amd.SOLVE_CLAMPED | umnn_amd.SOLVE_CAPPED | umnn_amd.SOLVE_NONFINITE)).any())
        assert mv.dim() == 0 and mv.is_cuda and np.isfinite(float(mv))
    if c.sweeps > c.d:          # (the eager test is met one sweep after the cap of d: record that many)
        torch._dynamo.reset()
        _, info = torch.compile(lambda z: c.m.invert(z, method="jacobi", context=c.ctx, sweep_tol=0, max_sweeps=c.sweeps, return_info=True),
                                backend="aot_eager", fullgraph=True)(c.z)
    for mv in info["last_move"]:
        _check_last_move(c, mv, f"compiled jacobi {name}")
    torch._dynamo.reset()
    ex = torch._dynamo.explain(fn)(c.z)
    assert ex.graph_break_count == 0 and ex.graph_count == 1
    code = ex.graphs[0].code
    assert _count(code, "cc_solve_block") == c.nb_flow * c.d and _count(code, "cc_solve") == 0


def test_compiled_single_block_and_sample():
    """A UMNNMAF block on its own, and ``sample(n)`` without a generator (the noise is drawn inside the graph)."""
    c = _case("d5")
    blk = c.m.nets[0]
    x_hat, info = torch.compile(lambda z: blk.invert(z, method="jacobi", sweep_tol=0, max_sweeps=c.d, return_info=True),
                                backend="aot_eager", fullgraph=True)(c.z)
    _check_round_trip(c.m, c.x, c.ctx, c.z, c.bound, x_hat, "compiled jacobi, one block")
    assert info["sweeps"] == c.d and info["status"].shape == c.z.shape and info["last_move"].dim() == 0
    torch._dynamo.reset()
    for kw in (dict(method="newton"), dict(method="jacobi", sweep_tol=0, max_sweeps=c.d)):
        s = torch.compile(lambda: c.m.sample(11, **kw), backend="aot_eager", fullgraph=True)()
        assert s.shape == (11, c.d) and s.device == c.z.device and torch.isfinite(s).all()
        torch._dynamo.reset()


def test_what_stays_eager():
    c = _case("d7")
    with pytest.raises(RuntimeError, match="invert cannot be traced by torch.jit.trace"):
        torch.jit.trace(lambda z: c.m.invert(z, method="newton"), c.z, check_trace=False)
    with torch.no_grad():
        want = c.m.invert(c.z, 5)
        got = torch.compile(lambda z: c.m.invert(z, 5), backend="aot_eager")(c.z)
    _same(got, want)
    torch._dynamo.reset()
    # the data-dependent sweeps are not recorded: fullgraph refuses them, without it the eager result comes back
    with torch.no_grad():
        want = c.m.invert(c.z, method="jacobi")
        got = torch.compile(lambda z: c.m.invert(z, method="jacobi"), backend="aot_eager")(c.z)
    _same(got, want)
    torch._dynamo.reset()
    with pytest.raises(Exception):
        torch.compile(lambda z: c.m.invert(z, method="jacobi", max_sweeps=3), backend="aot_eager", fullgraph=True)(c.z)


def test_eager_invert_dispatches_no_umnn_op():
    from torch.utils._python_dispatch import TorchDispatchMode

    class Rec(TorchDispatchMode):
        def __init__(self):
            super().__init__()
            self.names = set()

        def __torch_dispatch__(self, func, types, args=(), kwargs=None):
            self.names.add(str(func))
            return func(*args, **(kwargs or {}))

    c = _case("d7")
    with Rec() as rec, torch.no_grad():
        c.m.invert(c.z, 3)
        c.m.invert(c.z, method="newton")
        c.m.invert(c.z, method="jacobi", sweep_tol=0, max_sweeps=2)
        c.m.sample(5)
    assert rec.names and not any("umnn" in n for n in rec.names), sorted(n for n in rec.names if "umnn" in n)


# ---------------------------------------------------------------------------------------------------------------- 3. export
class _Sample(torch.nn.Module):
    def __init__(self, flow):
        super().__init__()
        self.flow = flow

    def forward(self, z):
        return self.flow.invert(z, method="jacobi", sweep_tol=0, max_sweeps=4)


def test_export_with_a_dynamic_batch():
    """d = 3 and four sweeps: at least d, the sequential answer by construction."""
    c = _case("d3")
    batch = torch.export.Dim("batch", min=2, max=4096)
    ep = torch.export.export(_Sample(c.m), (c.z,), dynamic_shapes=({0: batch},))
    assert "torch.ops.umnn.cc_solve_block" in ep.graph_module.print_readable(print_output=False)
    masked = 0
    for gm in ep.graph_module.modules():
        if isinstance(gm, torch.fx.GraphModule):
            for node in gm.graph.nodes:
                if node.op == "call_function" and node.target is torch.ops.aten.mul.Tensor:
                    masked += any(isinstance(a, torch.fx.Node) and a.op == "placeholder" and "mask" in a.name for a in node.args)
    print(f"multiplications with a mask buffer as operand: {masked}")
    assert 1 <= masked <= c.made_layers * c.nb_flow
    B2 = 50
    x2 = (1.5 * torch.randn(B2, c.d, generator=torch.Generator().manual_seed(B2))).to(DEV)
    with torch.no_grad():
        z2 = c.m(x2)
        x_hat = ep.module()(z2)
    assert umnn_amd.path_taken() == "hip"
    _check_round_trip(c.m, x2, None, z2, _flow_bound(c.m, x2, None), x_hat, "exported jacobi at a second batch size")


# ---------------------------------------------------------------------------------------------------------------- 4. GraphedSampler
@pytest.mark.parametrize("method", ["newton", "jacobi"])
@pytest.mark.parametrize("name", sorted(FLOWS))
def test_graphed_sampler_round_trip(name, method):
    c = _case(name)
    opts = dict(sweep_tol=0, max_sweeps=c.d) if method == "jacobi" else {}
    before = _launches()
    sampler = umnn_amd.GraphedSampler(c.m, c.B, context=c.ctx, method=method, **opts)
    captured = _launches()
    assert captured - before >= 2 * c.nb_flow * (c.d if method == "newton" else 1), "the warm-up and the capture both launch"
    assert sampler.captures == 1 and umnn_amd.path_taken() == "hip"
    x1 = sampler(z=c.z, context=c.ctx).clone()
    x2 = sampler(z=c.z, context=c.ctx)
    assert _launches() == captured, "a replay makes no launch from the host"
    _same(x1, x2)
    _check_round_trip(c.m, c.x, c.ctx, c.z, c.bound, x2, f"GraphedSampler {method} {name}")
    assert float((x2 - c.x_newton).abs().max()) <= 2 * c.bound
    if method == "jacobi":
        assert sampler.last_move.dim() == 0 and np.isfinite(float(sampler.last_move))
        if c.sweeps > c.d:
            longer = umnn_amd.GraphedSampler(c.m, c.B, context=c.ctx, method="jacobi", sweep_tol=0, max_sweeps=c.sweeps)
            longer(z=c.z, context=c.ctx)
            _check_last_move(c, longer.last_move, f"GraphedSampler jacobi {name}, {c.sweeps} sweeps")
        else:
            _check_last_move(c, sampler.last_move, f"GraphedSampler jacobi {name}")
    else:
        assert sampler.last_move is None
    if c.ctx is None:
        s = sampler()
        assert s.shape == (c.B, c.d) and torch.isfinite(s).all() and not torch.equal(s, x1)
    assert sampler.captures == 1


def test_graphed_sampler_of_a_single_block():
    c = _case("d5")
    blk = c.m.nets[0]
    for method, opts in (("newton", {}), ("jacobi", dict(sweep_tol=0, max_sweeps=c.d))):
        sampler = umnn_amd.GraphedSampler(blk, c.B, method=method, **opts)
        _check_round_trip(c.m, c.x, None, c.z, c.bound, sampler(z=c.z), f"GraphedSampler {method}, one block")


@pytest.mark.parametrize("how", ["optimizer_step", "load_state_dict"])
def test_graphed_sampler_recaptures_when_weights_move(how):
    c = _case("d7")
    m = copy.deepcopy(c.m)
    umnn_amd.invalidate_caches(m)
    sampler = umnn_amd.GraphedSampler(m, c.B, method="jacobi", sweep_tol=0, max_sweeps=c.d)
    x_old = sampler(z=c.z).clone()
    if how == "optimizer_step":
        params = [p for n, p in m.named_parameters() if "scaling" not in n]
        for p in params:
            p.requires_grad_(True)
        opt = torch.optim.SGD(params, lr=0.05)
        (-m.compute_ll(c.x)[0].mean()).backward()
        opt.step()
        opt.zero_grad(set_to_none=True)
        for p in params:
            p.requires_grad_(False)
    else:
        other = _make_flow(**{k: v for k, v in FLOWS["d7"].items() if k != "B"} | {"seed": 99})
        m.load_state_dict(other.state_dict())
    with torch.no_grad():
        z = m(c.x)
    x_hat = sampler(z=z)
    assert sampler.captures == 2
    assert not torch.equal(z, c.z)
    _check_round_trip(m, c.x, None, z, _flow_bound(m, c.x, None), x_hat, f"GraphedSampler after {how}")
    assert not torch.equal(x_hat, x_old)
    sampler(z=z)
    assert sampler.captures == 2
    sampler.refresh()
    assert sampler.captures == 3
    _check_round_trip(m, c.x, None, z, _flow_bound(m, c.x, None), sampler(z=z), "GraphedSampler after refresh()")


def test_graphed_sampler_refuses_what_it_cannot_capture():
    import warnings
    m = _make_flow(3, [80] * 6, 4, 20, 1, seed=5)       # (no in-kernel solve for this integrand: the host-driven loop reads the device)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        for method, opts in (("newton", {}), ("jacobi", dict(sweep_tol=0, max_sweeps=3))):
            with pytest.raises(ValueError, match="needs the in-kernel solve"):
                umnn_amd.GraphedSampler(m, 9, method=method, **opts)
    c = _case("d2")
    with pytest.raises(ValueError, match="sweep_tol=0 and max_sweeps"):
        umnn_amd.GraphedSampler(c.m, c.B, method="jacobi")
    with pytest.raises(ValueError, match="sweep_tol=0 and max_sweeps"):
        umnn_amd.GraphedSampler(c.m, c.B, method="jacobi", sweep_tol=1e-6, max_sweeps=2)
    with pytest.raises(ValueError, match="'newton' or 'jacobi'"):
        umnn_amd.GraphedSampler(c.m, c.B, method="bracket")
