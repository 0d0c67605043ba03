"""Sample with log-density on the device: ``umnn_cc_solve_lj`` (the solve kernel's epilogue adds log(f(x) + 1e-10) + s to a running row
sum), the glue kernels ``umnn_flow_sample_lj_rows`` / ``umnn_flow_sample_ll``, ``invert(..., return_log_jac=True)`` and
``sample_and_log_prob`` on every method and arithmetic mode, their launch counts and their recorded forms.

Yardsticks.  Kernel level: the f_x of ``want_info`` calls of the same solve, summed in float64 -- the terms are the same numbers, so only
the fast log's last bits and the fp32 running sum differ: 1e-5 d.  Flow level: a float64 CPU copy of the flow evaluated at the returned x
(the ATen path, which predates these entry points), at the project's parity bar 1e-4 max(1, |truth|); ``flow.log_prob(x)`` on the device
is held to the same bar in the same test.  Measured maxima: EXPERIMENTS.md ("Sample with log-density")."""
import copy
import ctypes
import warnings

import pytest
import torch
import torch._dynamo

import umnn_amd
from tests import _fwd_plan_cases as P
from tests import _sample_log_prob_cases as C
from umnn_amd import _lib, integral as I
from umnn_amd.nets import mlp_spec

pytestmark = pytest.mark.gpu
TOL = 1e-4
MODES = ["f16x3", "bf16x3", "bf16x6", "fp32"]
DEV = torch.device("cuda:0")


@pytest.fixture(autouse=True)
def _fresh():
    torch._dynamo.reset()
    old = umnn_amd.get_forward_precision(), umnn_amd.get_backward_precision()
    yield
    torch._dynamo.reset()
    umnn_amd.set_forward_precision(old[0])
    umnn_amd.set_backward_precision(old[1])


def _kname():
    return _lib.lib().umnn_last_kernel_name().decode()


# ------------------------------------------------------------------------------------------------------------ 1. kernel level
SOLVE_IDS = ["solve-50x4", "solve-100x3", "solve-wide-first-7-13", "solve-bf16x6-50x4", "solve-bf16x3-50x4", "solve-few-nodes",
             "solve-dozens-of-rows"]
_BY_ID = {c["id"]: c for c in P.CASES}


def _lj_reference(fxs, s_terms):
    """sum_j [log(f_x_j + 1e-10) + s_j] in float64 from the fp32 f_x of the ``want_info`` calls."""
    total = torch.zeros(fxs[0].shape[0], dtype=torch.float64)
    for fx, s in zip(fxs, s_terms):
        total += torch.log(fx.double().cpu() + 1e-10) + s
    return total


def _solve_every_dimension(spec, h, t, n, scaling=None, scale_row=None, garbage=float("nan")):
    """umnn_cc_solve (want_info) and umnn_cc_solve_lj for j = 0..d-1 -> (x_ref, [f_x_j], [status_j], x, [f_x_j], [status_j], lj_row);
    lj_first is set on the first call only, on a buffer full of ``garbage``."""
    B, d = t.shape
    x_ref, x = torch.zeros_like(t), torch.zeros_like(t)
    lj = torch.full((B,), garbage, device=t.device)
    ref, new = ([], []), ([], [])
    for j in range(d):
        kw = dict(j=j, scaling=scaling, scale_row=scale_row, off_h0=True, max_iter=32)
        before = _lib.lib().umnn_launch_count()
        out = I.hip_solve(spec, h, t, n, x_out=x_ref, **kw)
        assert out is not None and _lib.lib().umnn_launch_count() - before == 1
        name = _kname()
        ref[0].append(out[1]), ref[1].append(out[2])
        out = I.hip_solve(spec, h, t, n, x_out=x, lj_row=lj, lj_first=j == 0, **kw)
        assert out is not None and _lib.lib().umnn_launch_count() - before == 2 and _kname() == name, "the same launch and kernel"
        new[0].append(out[1]), new[1].append(out[2])
    return x_ref, ref[0], ref[1], x, new[0], new[1], lj


@pytest.mark.parametrize("rows", ["all", "one"])
@pytest.mark.parametrize("cid", SOLVE_IDS)
def test_solve_lj_adds_the_rows_log_jacobian_in_the_same_launch(cid, rows):
    c = _BY_ID[cid]
    net, t, h, scaling = (v.to(DEV) for v in P.inputs(c))
    if rows == "one":
        t, h = t[:1].contiguous(), h[:1].contiguous()
    B, d = t.shape
    spec = mlp_spec(net)
    scale_row = torch.exp(0.3 * torch.randn(B, generator=torch.Generator().manual_seed(B))).to(DEV)
    with _lib.options(**c["options"]):
        for variant in ("scaling", "scale_row", "none"):
            kw = dict(scaling=scaling) if variant == "scaling" else dict(scale_row=scale_row) if variant == "scale_row" else {}
            # (lj_first = 1 overwrites garbage: NaN in the whole buffer, and a huge finite value)
            for garbage in (float("nan"), 3e38) if variant == "scaling" else (float("nan"),):
                x_ref, fx_ref, st_ref, x, fx, st, lj = _solve_every_dimension(spec, h, t, c["n"], garbage=garbage, **kw)
                if rows == "all":
                    assert _kname() == c["name"], _kname()
                assert torch.equal(x, x_ref), "x is umnn_cc_solve's bit for bit"
                for j in range(d):
                    assert torch.equal(st[j], st_ref[j]) and torch.equal(fx[j], fx_ref[j])
                    assert not ((st[j] & umnn_amd.SOLVE_NONFINITE) != 0).any()
                s_terms = [float(scaling[j]) if variant == "scaling" else torch.log(scale_row.double().cpu()) if variant == "scale_row"
                           else 0. for j in range(d)]
                want = _lj_reference(fx_ref, s_terms)
                err = float((lj.double().cpu() - want).abs().max())
                print(f"{cid} rows={rows} {variant}: max |lj_row - sum| {err:.2e} (bound {1e-5 * d:.0e})")
                assert torch.isfinite(lj).all() and err <= 1e-5 * d


def test_overflow_protocol_counts_every_row_once():
    """f16x3 with rows whose embedding overflows the fp16 pieces (tests/test_gpu_solve_coverage.py's construction: those rows of h times
    3e6): they are deferred to the queued bf16 build, which adds their term; every other row is added by the fp16 build."""
    c = _BY_ID["solve-50x4"]
    net, t, h, scaling = (v.to(DEV) for v in P.inputs(c))
    B, d = t.shape
    spec = mlp_spec(net)
    hot = torch.zeros(B, dtype=torch.bool, device=DEV)
    hot[[0, 1, 2, 20, B - 1]] = True                      # (first tile, a middle tile, the five-lane tail tile)
    h = h.clone()
    h[hot] *= 3e6
    t = torch.randn(B, d, generator=torch.Generator().manual_seed(2)).to(DEV)
    umnn_amd.set_forward_precision("bf16x3")
    xb, fxb, _, _, _, _, ljb = _solve_every_dimension(spec, h, t, c["n"], scaling=scaling)
    assert _kname().startswith("cc_solve_bf16<")
    umnn_amd.set_forward_precision("f16x3")
    x_ref, fx_ref, st_ref, x, fx, st, lj = _solve_every_dimension(spec, h, t, c["n"], scaling=scaling)
    assert _kname().startswith("cc_solve_f16<")
    # deferred rows carry the bf16 build's numbers bit for bit; the others are the fp16 build's, which differ from them somewhere
    assert bool(hot.any()) and bool((~hot).any())
    assert torch.equal(x_ref[hot], xb[hot]) and all(torch.equal(a[hot], b[hot]) for a, b in zip(fx_ref, fxb)), "no row was deferred"
    assert not torch.equal(x_ref[~hot], xb[~hot]), "every row was deferred"
    assert torch.equal(x, x_ref) and all(torch.equal(a, b) for a, b in zip(st, st_ref))
    want = _lj_reference(fx_ref, [float(scaling[j]) for j in range(d)])
    got = lj.double().cpu()
    err = (got - want).abs()
    print(f"overflow protocol: max |lj_row - sum| {float(err.max()):.2e} deferred rows {float(err[hot.cpu()].max()):.2e}; "
          f"min |sum| {float(want.abs().min()):.2e}")
    assert float(want.abs().min()) > 1e-3, "a sum near zero could hide a row counted twice or not at all"
    assert float(err.max()) <= 1e-5 * d, "every row once: neither zero nor doubled"
    assert torch.equal(lj[hot], ljb[hot]), "deferred rows: the queued build's own sum"


@pytest.mark.parametrize("precision", MODES)
def test_nan_target_poisons_its_own_row_only(precision):
    c = _BY_ID["solve-50x4"]
    net, t, h, scaling = (v.to(DEV) for v in P.inputs(c))
    t = t.clone()
    t[5, 1] = float("nan")
    umnn_amd.set_forward_precision(precision)
    x_ref, fx_ref, st_ref, x, fx, st, lj = _solve_every_dimension(mlp_spec(net), h, t, c["n"], scaling=scaling)
    keep = torch.ones(t.shape[0], dtype=torch.bool)
    keep[5] = False
    assert torch.isnan(lj[5]) and torch.isfinite(lj[keep.to(DEV)]).all()
    assert bool((st[1][5] & umnn_amd.SOLVE_NONFINITE) != 0) and torch.equal(x[keep.to(DEV)], x_ref[keep.to(DEV)])
    want = _lj_reference([f[keep.to(DEV)] for f in fx_ref], [float(scaling[j]) for j in range(t.shape[1])])
    assert float((lj.double().cpu()[keep] - want).abs().max()) <= 1e-5 * t.shape[1]


# ------------------------------------------------------------------------------------------------------------ 2. glue kernels
@pytest.mark.parametrize("first", [0, 1])
@pytest.mark.parametrize("B,d", [(1, 1), (5, 3), (37, 63), (3, 784)])
def test_glue_kernels_against_float64(B, d, first):
    """fp32 terms summed lane-strided and by a six-step butterfly: per row at most (2 + d / 64 + 6) roundings of 6e-8 relative to the sum
    of the terms' magnitudes -- 2e-6 (sum |terms| + |previous|) + 1e-6 covers d = 784."""
    g = torch.Generator().manual_seed(100 * B + d)
    fx = torch.exp(torch.randn(B, d, generator=g)).to(DEV)
    fx[0, 0] = 0.                                                # (log(0 + 1e-10): the epsilon's case)
    scaling = (0.3 * torch.randn(d, generator=g)).to(DEV)
    z = torch.randn(B, d, generator=g).to(DEV)
    prev = torch.randn(B, generator=g).to(DEV)
    lj = prev.clone() if not first else torch.full((B,), float("nan"), device=DEV)
    rc = _lib.lib().umnn_flow_sample_lj_rows(I._ptr(fx), I._ptr(scaling), B, d, first, I._ptr(lj), I._stream(DEV))
    assert rc == 0
    terms = torch.log(fx.double().cpu() + 1e-10) + scaling.double().cpu()
    want = terms.sum(1) + (0. if first else prev.double().cpu())
    bound = 2e-6 * (terms.abs().sum(1) + (0. if first else prev.double().cpu().abs())) + 1e-6
    assert bool(((lj.double().cpu() - want).abs() <= bound).all()), float((lj.double().cpu() - want).abs().max())
    ll = torch.empty(B, device=DEV)
    assert _lib.lib().umnn_flow_sample_ll(I._ptr(z), I._ptr(lj), B, d, I._ptr(ll), I._stream(DEV)) == 0
    gauss = .5 * (1.8378770664093453 + z.double().cpu() ** 2)
    want_ll = lj.double().cpu() - gauss.sum(1)
    bound = 2e-6 * (gauss.sum(1) + lj.double().cpu().abs()) + 1e-6
    assert bool(((ll.double().cpu() - want_ll).abs() <= bound).all()), float((ll.double().cpu() - want_ll).abs().max())
    # the host wrappers are these launches
    assert torch.equal(I.sample_ll(z, lj), ll)
    assert torch.equal(I.sample_lj_rows(fx, scaling, None if first else prev.clone()), lj)


def test_glue_kernels_empty_batch_launches_nothing():
    p = ctypes.c_void_p(0)
    assert _lib.lib().umnn_flow_sample_lj_rows(p, p, 0, 3, 1, p, I._stream(DEV)) == 0
    assert _lib.lib().umnn_flow_sample_ll(p, p, 0, 3, p, I._stream(DEV)) == 0
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------------------ 3. flow level
GPU_METHODS = {"newton": dict(method="newton"), "newton-progressive": dict(method="newton", conditioner="progressive"),
               "jacobi": dict(method="jacobi", sweep_tol=0),          # (max_sweeps = d: the sequential answer by construction)
               # sixteen rounds: the bracket is below fp32 resolution, so z against T(x) is the solve's residual as in the other methods
               # (the default ten leave 100 (2 / 9)^10 = 3e-5 of bracket, which the Gaussian term would see)
               "bracket": dict(method="bracket", iter=16)}
_FLOWS = {}


def _gpu_flow(name):
    """(fp32 flow on the device, z, context, its float64 CPU copy): the CPU file's flows, plus one MNIST-family net at d = 5."""
    if name not in _FLOWS:
        if name == "mnist-family":
            torch.manual_seed(5)
            m = umnn_amd.UMNNMAFFlow(nb_flow=2, nb_in=5, hidden_derivative=[100, 50, 50], hidden_embedding=[64, 64], embedding_s=8,
                                     nb_steps=30, solver="CCParallel").eval()
            with torch.no_grad():
                for blk in m.nets:
                    blk.scaling.copy_(0.3 * torch.randn(5))
            z, ctx = torch.randn(C.B, 5), None
        else:
            m64, z, ctx = C.flow(name)
            m = copy.deepcopy(m64).float()
            umnn_amd.invalidate_caches(m)
        for p in m.parameters():
            p.requires_grad_(False)
        truth = copy.deepcopy(m).double().cpu()
        umnn_amd.invalidate_caches(truth)
        m = m.to(DEV)
        _FLOWS[name] = (m, z.float().to(DEV), None if ctx is None else ctx.float().to(DEV), truth)
    return _FLOWS[name]


def _opts(method, d):
    o = dict(GPU_METHODS[method])
    if o["method"] == "jacobi":
        o["max_sweeps"] = d
    return o


def _rel(a, truth):
    return float(((a.double().cpu() - truth).abs() / truth.abs().clamp(min=1.)).max())


@pytest.mark.parametrize("precision", MODES)
@pytest.mark.parametrize("name", [f[0] for f in C.FLOWS] + ["mnist-family"])
def test_flow_log_density_against_the_float64_cpu_flow(name, precision):
    m, z, ctx, truth = _gpu_flow(name)
    umnn_amd.set_forward_precision(precision)
    for method in GPU_METHODS:
        o = _opts(method, z.shape[1])
        with torch.no_grad():
            x0 = m.invert(z, context=ctx, **o)
            x, lj = m.invert(z, context=ctx, return_log_jac=True, **o)
            assert umnn_amd.path_taken() == "hip"
            assert torch.equal(x, x0), f"{method}: the flag must not change x"
            lp = I.sample_ll(z, lj)
            ll64 = truth.compute_ll(x.double().cpu(), None if ctx is None else ctx.double().cpu())[0]
            own = m.log_prob(x, ctx)
        e_new, e_own = _rel(lp, ll64), _rel(own, ll64)
        print(f"{name} {precision} {method}: sample_and_log_prob {e_new:.2e}, log_prob(x) {e_own:.2e} of max(1, |truth|)")
        assert lp.shape == (C.B,) and lp.dtype == torch.float32
        assert e_own <= TOL, f"{method}: the yardstick itself"
        assert e_new <= TOL, method


@pytest.mark.parametrize("name", ["f2-d3", "cond", "mnist-family"])
def test_sample_and_log_prob_is_sample_with_its_density(name):
    m, z, ctx, truth = _gpu_flow(name)
    for method in GPU_METHODS:
        o = _opts(method, z.shape[1])
        x0 = m.sample(C.B, context=ctx, generator=torch.Generator(device=DEV).manual_seed(3), **o)
        x, lp = m.sample_and_log_prob(C.B, context=ctx, generator=torch.Generator(device=DEV).manual_seed(3), **o)
        assert torch.equal(x, x0) and lp.shape == (C.B,) and not lp.requires_grad
        with torch.no_grad():
            ll64 = truth.compute_ll(x.double().cpu(), None if ctx is None else ctx.double().cpu())[0]
        assert _rel(lp, ll64) <= TOL, method
    x, lp = m.sample_and_log_prob(0, context=None if ctx is None else ctx[:0])
    assert x.shape == (0, z.shape[1]) and lp.shape == (0,)
    blk = m.nets[0]
    xb, lpb = blk.sample_and_log_prob(C.B, context=ctx, generator=torch.Generator(device=DEV).manual_seed(4))
    with torch.no_grad():
        ref = truth.nets[0].compute_ll(xb.double().cpu(), None if ctx is None else ctx.double().cpu())[0]
    assert _rel(lpb, ref) <= TOL


@pytest.mark.parametrize("method", ["newton", "newton-progressive", "jacobi"])
def test_nan_noise_poisons_the_density_of_its_own_sample_only(method):
    m, z, ctx, _ = _gpu_flow("f2-d3")
    o = _opts(method, 3)
    bad = z.clone()
    bad[2, 1] = float("nan")
    with torch.no_grad():
        x, lj = m.invert(z, return_log_jac=True, **o)
        xb, ljb = m.invert(bad, return_log_jac=True, **o)
    keep = torch.ones(C.B, dtype=torch.bool, device=DEV)
    keep[2] = False
    assert torch.isnan(ljb[2]) and torch.isnan(xb[2]).any()
    assert torch.equal(xb[keep], x[keep]) and torch.equal(ljb[keep], lj[keep]), "the rows of a batch are independent"


ROWS = 17       # one full 16-row tile plus one row


def _rows(name):
    """``_gpu_flow(name)`` with ROWS rows of noise (and context) in place of the shared six."""
    m, z, ctx, truth = _gpu_flow(name)
    g = torch.Generator().manual_seed(17)
    z = torch.randn(ROWS, z.shape[1], generator=g).to(DEV)
    return m, z, None if ctx is None else torch.randn(ROWS, ctx.shape[1], generator=g).to(DEV), truth


@pytest.mark.parametrize("method", list(GPU_METHODS))
@pytest.mark.parametrize("name", ["f1-d3", "f3-d3", "cond"])
def test_one_x_whatever_is_asked_for(name, method):
    m, z, ctx, _ = _rows(name)
    o = _opts(method, z.shape[1])
    C.check_one_x(m, len(m.nets), z, ctx, o)
    C.check_one_x(m.nets[0], None, z, ctx, o)
    assert umnn_amd.path_taken() == "hip"


@pytest.mark.parametrize("method", list(GPU_METHODS))
@pytest.mark.parametrize("name", ["f2-d3", "f3-d5", "cond"])
def test_flow_invert_is_the_block_inverts_composed(name, method):
    """x is the blocks' x bit for bit; log_jac is the same fp32 terms added in another order ("newton": the solve launches of every block
    add into one running sum; the composition adds per-block sums).  Two orders of adding n = nb_flow d terms differ by at most
    2 (n - 1) eps sum |terms| (each order is within (n - 1) eps sum |terms| of the exact sum), eps = 1.2e-7 and sum |terms| from the
    float64 CPU flow's ``_transform`` at x: 1.2e-6 to 3.3e-6 of sum |terms| for these flows.  Measured: 3.8e-8 to 6.7e-8 of sum |terms| ("newton", both conditioners), 0 ("jacobi", "bracket")."""
    m, z, ctx, truth = _rows(name)
    o = _opts(method, z.shape[1])
    with torch.no_grad():
        x, lj = m.invert(z, context=ctx, return_log_jac=True, **o)
        xc, ljc = C.composed(m, z, ctx, o)
    assert torch.equal(xc, x) and umnn_amd.path_taken() == "hip"
    n = len(m.nets) * z.shape[1]
    mag = C.lj_magnitude(truth, x, None if ctx is None else ctx.double().cpu())
    err = ((lj - ljc).abs().double().cpu() / mag).max()
    print(f"{name} {method}: |lj - composed| / sum |terms| {float(err):.2e} (bound {2 * (n - 1) * torch.finfo(torch.float32).eps:.1e})")
    assert lj.dtype == ljc.dtype == torch.float32 and float(err) <= 2 * (n - 1) * torch.finfo(torch.float32).eps


def test_mid_walk_fallback_keeps_its_density():
    """An integrand with a single hidden layer: the solve kernels refuse it (UMNN_EUNSUPPORTED at the first dimension of each block), the
    rest of the block runs the Newton iteration from the host on ``hip_forward`` and the running log_jac goes on in torch ops."""
    torch.manual_seed(9)
    d = 3
    m = umnn_amd.UMNNMAFFlow(nb_flow=2, nb_in=d, hidden_derivative=[50], hidden_embedding=[16, 16], embedding_s=3, nb_steps=20,
                             solver="CCParallel").eval()
    with torch.no_grad():
        for blk in m.nets:
            blk.scaling.copy_(0.3 * torch.randn(d))
    for p in m.parameters():
        p.requires_grad_(False)
    truth = copy.deepcopy(m).double()
    m = m.to(DEV)
    z = torch.randn(ROWS, d).to(DEV)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)          # (the refusal is announced once)
        x0 = m.invert(z, method="newton")
        before = _lib.lib().umnn_launch_count()
        x, lj = m.invert(z, method="newton", return_log_jac=True)
        launches = _lib.lib().umnn_launch_count() - before
    assert umnn_amd.path_taken() == "hip" and torch.equal(x, x0)
    assert launches > len(m.nets) * d, "the host-driven loop launches one quadrature per iteration"
    with torch.no_grad():
        ref = truth.compute_log_jac(x.double().cpu()).sum(1)
    err = _rel(lj, ref)
    print(f"fallback: {launches} launches, log_jac against the float64 CPU flow {err:.2e}")
    assert lj.shape == (ROWS,) and lj.dtype == torch.float32 and err <= TOL


# ------------------------------------------------------------------------------------------------------------ 4. launch counts
def _deltas(fn):
    lib = _lib.lib()
    q0, c0 = lib.umnn_launch_count(), lib.umnn_made_launch_count()
    fn()
    return lib.umnn_launch_count() - q0, lib.umnn_made_launch_count() - c0


@pytest.mark.parametrize("name", ["f2-d3", "f3-d5", "cond"])
def test_launch_counts(name):
    m, z, ctx, _ = _gpu_flow(name)
    nb_flow, d = len(m.nets), z.shape[1]
    for method in GPU_METHODS:
        o = _opts(method, d)
        m.sample(C.B, context=ctx, **o), m.sample_and_log_prob(C.B, context=ctx, **o)          # (caches, tables, plans)
        plain = _deltas(lambda: m.sample(C.B, context=ctx, **o))
        both = _deltas(lambda: m.sample_and_log_prob(C.B, context=ctx, **o))
        print(f"{name} {method}: sample {plain}, sample_and_log_prob {both} (quadrature launches, conditioner launches)")
        assert both[0] == plain[0] + (nb_flow if method == "bracket" else 0), method
        assert both[1] == plain[1], method
        if o["method"] == "newton":
            assert plain[0] == nb_flow * d


# ------------------------------------------------------------------------------------------------------------ 5. graph modes
def _flow_bound(truth, x, ctx):
    """sum over blocks of TOL / min exp(s) f from the float64 copy's own log_jac (tests/test_gpu_graph_sampling._flow_bound)."""
    xi = x.detach().cpu().double()
    c64 = None if ctx is None else ctx.detach().cpu().double()
    total = 0.
    with torch.no_grad():
        for blk in truth.nets:
            zz, lj = blk._transform(xi, c64, want_jac=True)
            total += TOL / float(torch.exp(lj.min()))
            xi = torch.flip(zz, [1])
    return total


def _matches_eager(tag, got, eager, bound):
    (x, lj), (xe, lje) = got, eager
    ex, el = float((x - xe).abs().max()), _rel(lj, lje.double().cpu())
    print(f"{tag}: |x - eager| {ex:.2e} (bound {2 * bound:.2e}), log_jac against eager {el:.2e}")
    assert x.shape == xe.shape and lj.shape == lje.shape and lj.dtype == torch.float32
    assert ex <= 2 * bound and el <= TOL, tag


class _Module(torch.nn.Module):
    def __init__(self, flow):
        super().__init__()
        self.flow = flow

    def forward(self, z):
        return self.flow.invert(z, method="jacobi", sweep_tol=0, max_sweeps=3, return_log_jac=True)


def test_compiled_and_exported_forms_match_eager():
    m, z, ctx, truth = _gpu_flow("f2-d3")
    with torch.no_grad():
        eager_n = m.invert(z, method="newton", return_log_jac=True)
        eager_j = m.invert(z, method="jacobi", sweep_tol=0, max_sweeps=3, return_log_jac=True)
    bound = _flow_bound(truth, eager_n[0], None)
    got = torch.compile(lambda t: m.invert(t, method="newton", return_log_jac=True), backend="aot_eager", fullgraph=True)(z)
    _matches_eager("compiled newton", got, eager_n, bound)
    torch._dynamo.reset()
    got = torch.compile(lambda t: m.invert(t, method="jacobi", sweep_tol=0, max_sweeps=3, return_log_jac=True), backend="aot_eager",
                        fullgraph=True)(z)
    _matches_eager("compiled jacobi", got, eager_j, bound)
    torch._dynamo.reset()
    x, info, lj = torch.compile(lambda t: m.invert(t, method="jacobi", sweep_tol=0, max_sweeps=3, return_info=True, return_log_jac=True),
                                backend="aot_eager", fullgraph=True)(z)
    assert info["sweeps"] == [3, 3]
    _matches_eager("compiled jacobi with info", (x, lj), eager_j, bound)
    torch._dynamo.reset()
    ep = torch.export.export(_Module(m), (z,))
    assert "torch.ops.umnn.cc_solve_block" in ep.graph_module.print_readable(print_output=False)
    with torch.no_grad():
        got = ep.module()(z)
    _matches_eager("exported jacobi", got, eager_j, bound)
    torch._dynamo.reset()
    x, lp = torch.compile(lambda: m.sample_and_log_prob(11), backend="aot_eager", fullgraph=True)()
    with torch.no_grad():
        ll64 = truth.compute_ll(x.double().cpu())[0]
    assert x.shape == (11, 3) and _rel(lp, ll64) <= TOL


@pytest.mark.parametrize("method", ["newton", "newton-progressive", "jacobi"])
def test_graphed_sampler_with_log_prob(method):
    m, z, ctx, truth = _gpu_flow("f2-d3")
    o = _opts(method, 3)
    with torch.no_grad():
        xe, lje = m.invert(z, return_log_jac=True, **o)
        lpe = I.sample_ll(z, lje)
    bound = _flow_bound(truth, xe, None)
    kw = {k: v for k, v in o.items() if k != "method"}
    sampler = umnn_amd.GraphedSampler(m, C.B, method=o["method"], log_prob=True, **kw)
    captured = _lib.lib().umnn_launch_count()
    for replay in range(2):
        x, lp = sampler(z=z)
        _matches_eager(f"GraphedSampler {method}, replay {replay}", (x, lp), (xe, lpe), bound)
    assert _lib.lib().umnn_launch_count() == captured, "a replay makes no launch from the host"
    x, lp = sampler()
    with torch.no_grad():
        ll64 = truth.compute_ll(x.double().cpu())[0]
    assert _rel(lp, ll64) <= TOL and sampler.captures == 1
    plain = umnn_amd.GraphedSampler(m, C.B, method=o["method"], **kw)
    assert torch.is_tensor(plain(z=z)), "without the flag a replay returns x alone"
