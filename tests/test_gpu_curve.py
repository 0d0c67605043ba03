"""Whole curves from one quadrature on the GPU (csrc/cc_multi.hip cc_fwd_multi_nodes_kernel, csrc/cc_cumulate.hip):
``MonotonicNN.forward_curve`` / ``cumulative_incidence`` and ``IntegralCurve`` against the float64 truth on every case, the end point
against ``forward``, launch counts and names, bit-identity across runs and precision settings, the ATen route under autograd, and
graph mode (torch.compile, torch.export, hipGraph capture).  Cases, truth, tolerance (1e-5) and kink margins: tests/_curve_cases.py."""
import copy
import warnings

import numpy as np
import pytest
import torch

import umnn_amd
from tests import _curve_cases as C
from tests import _util as U
from umnn_amd import _lib, integral as I
from umnn_amd.quadrature import cc_cumulative_matrix

pytestmark = pytest.mark.gpu
TOL = C.TOL
HIP_CASES = [i for i, c in enumerate(C.CASES) if c.K <= 16]
FAMILY = {0: "T=4,KS=13", 1: "T=4,KS=13", 2: "T=7,KS=26", 3: "T=8,KS=32", 5: "T=2,KS=8", 6: "T=4,KS=16"}
MT = {7: 1, 8: 1, 9: 1, 20: 2, 50: 4}


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


@pytest.fixture(autouse=True)
def _restore():
    old = umnn_amd.get_forward_precision(), umnn_amd.get_backward_precision()
    yield
    umnn_amd.set_forward_precision(old[0])
    umnn_amd.set_backward_precision(old[1])


def _kname():
    return _lib.lib().umnn_last_kernel_name().decode()


def _count():
    return _lib.lib().umnn_launch_count()


def _on(dev, model, *tensors):
    return (copy.deepcopy(model).to(dev),) + tuple(t.to(dev) for t in tensors)


def _curve(mg, xg, hg):
    with torch.no_grad():
        return mg.forward_curve(xg, hg, with_derivative=True)


def _errs(out, T, rows=None):
    pick = (lambda a: a) if rows is None else (lambda a: a[rows])
    return [U.rel_err(a.cpu().numpy(), pick(b)) for a, b in zip(out, (T.t, T.y, T.dy))]


# ------------------------------------------------------------------------------------------------------------ values
@pytest.mark.parametrize("i", HIP_CASES)
def test_forward_curve_matches_float64(dev, i):
    c = C.CASES[i]
    model, x, h = C.build(c)
    T = C.case_truth(i)
    mg, xg, hg = _on(dev, model, x, h)
    n0 = _count()
    t, y, dy = out = _curve(mg, xg, hg)
    assert _count() - n0 == 2 and I.path_taken() == "hip"                     # one node launch and one cumulate launch
    assert _kname() == f"cc_cumulate<MT={MT[c.nb_steps]}>"
    errs = _errs(out, T)
    print(f"case {i}: t {errs[0]:.2e} y {errs[1]:.2e} dy/dt {errs[2]:.2e}; margin {T.margin:.2e}")
    assert T.margin >= C.MIN_MARGIN
    assert t.shape == (c.B, c.nb_steps + 1) and y.shape == dy.shape == (c.B, c.nb_steps + 1, c.K)
    assert max(errs) <= TOL
    assert torch.equal(t[:, 0], torch.zeros_like(t[:, 0])) and torch.equal(t[:, -1:], xg)
    with torch.no_grad():
        yx = mg(xg, hg)
        n1 = _count()
        F, f_nodes = I.hip_forward_multi_nodes(I.mlp_spec(mg.integrand), None, xg, hg, c.nb_steps)
    assert _count() - n1 == 1 and _kname() == f"cc_fwd_multi_nodes<{FAMILY[i]},P=1>"
    end = U.rel_err(y[:, -1].cpu().numpy(), yx.cpu().numpy())
    print(f"case {i}: y[:, n] vs forward(x, h) {end:.2e}")
    assert end <= TOL
    # the node launch's own F is the forward's, and its nodes are dy/dt's in node order
    with torch.no_grad():
        F_fwd = I.aten_forward(mg.integrand, torch.zeros_like(xg), xg, hg, c.nb_steps) if c.K == 1 else I.hip_forward_multi(I.mlp_spec(mg.integrand), None, xg, hg, c.nb_steps)[0]
    assert U.rel_err(F.cpu().numpy(), F_fwd.cpu().numpy()) <= TOL and (c.K == 1 or torch.equal(F, F_fwd))
    o, ls = mg._offset_log_scaling(hg)
    assert torch.equal((torch.exp(ls).unsqueeze(1) * f_nodes.flip(1)), dy)


@pytest.mark.parametrize("i", HIP_CASES)
def test_cumulative_incidence_is_the_cumulated_integrand(dev, i):
    """The third launch: CIF = cumulate(hz exp(-sum_j H_j)) of the curve's own H and hz, at positive times.  The reference is the float64
    product of the same integrand with the float64 table.  On these untrained nets the integrand spans many magnitudes (exp of minus a
    sum of K offsets), so each row is measured against its own largest value, what the rounding error of a linear map scales with:
    (n + 1) 2^-24 sum_j |Q_ij| g_j, and with g > 0 and |Q_ij| of the order of the weights w_j that is about 2 (n + 1) 2^-24 <= 6.1e-6 of
    the row's end value in the worst case (n = 50): inside TOL."""
    c = C.CASES[i]
    model, x, h = C.build(c)
    mg, xg, hg = _on(dev, model, x.abs() + 0.5, h)
    t, H, hz = _curve(mg, xg, hg)
    n0 = _count()
    with torch.no_grad():
        t2, cif = mg.cumulative_incidence(xg, hg, curve=True)
    assert _count() - n0 == 3 and I.path_taken() == "hip" and _kname() == f"cc_cumulate<MT={MT[c.nb_steps]}>"     # one more cumulate launch
    with torch.no_grad():
        end = mg.cumulative_incidence(xg, hg)
        g = (hz * torch.exp(-H.sum(2, keepdim=True))).double().cpu()
    Q = torch.as_tensor(cc_cumulative_matrix(c.nb_steps)[::-1, ::-1].copy())
    ref = torch.einsum("ij,bjk->bik", Q, g) * (xg.double().cpu() / 2).unsqueeze(2)
    err = float(((cif.double().cpu() - ref).abs().amax((1, 2)) / ref.abs().amax((1, 2)).clamp(min=1.)).max())
    print(f"case {i}: CIF vs the float64 product of its integrand, per row {err:.2e}")
    assert cif.shape == (c.B, c.nb_steps + 1, c.K) and torch.equal(t2, t) and err <= TOL
    assert torch.equal(end, cif[:, -1]) and torch.equal(cif[:, 0], torch.zeros_like(cif[:, 0]))


def test_cumulative_incidence_matches_float64(dev):
    """The well-conditioned case of test_curve_cpu (4 rows, K = 2, n = 50, positive times), against the float64 model on the CPU --
    itself held to the nested composite rule there."""
    model, x, h = C.build(C.CIF_CASE)
    x = x.abs() + 0.5
    with torch.no_grad():
        ref = copy.deepcopy(model).double().cumulative_incidence(x.double(), h.double(), curve=True)[1]
    mg, xg, hg = _on(dev, model, x, h)
    with torch.no_grad():
        cif = mg.cumulative_incidence(xg, hg, curve=True)[1]
    err = U.rel_err(cif.cpu().numpy(), ref.numpy())
    print(f"CIF case: {err:.2e}")
    assert I.path_taken() == "hip" and err <= TOL


def test_p2_variant_with_a_ragged_last_group(dev):
    cus = torch.cuda.get_device_properties(dev).multi_processor_count
    model, x, h, idx = C.p2_case(cus)
    T = C.p2_truth()
    assert T.margin >= C.MIN_MARGIN and x.shape[0] == 2 * 4 * cus * 16 + 5
    mg, xg, hg = _on(dev, model, x, h)
    out = _curve(mg, xg, hg)
    with torch.no_grad():
        I.hip_forward_multi_nodes(I.mlp_spec(mg.integrand), None, xg, hg, 7)
    assert _kname() == "cc_fwd_multi_nodes<T=2,KS=8,P=2>"
    errs = _errs(out, T, idx.numpy())
    print(f"P = 2, B = {x.shape[0]}: t {errs[0]:.2e} y {errs[1]:.2e} dy/dt {errs[2]:.2e}")
    assert max(errs) <= TOL
    # every copy of a base row carries that row's bits, wherever in a group it sits
    for a in out:
        assert torch.equal(a, a[:C.P2_BASE.B][idx.to(dev)])


def test_operator_with_nonzero_x0(dev):
    net, x, h, _ = C.M.build(C.X0_CASE)
    x0, n = C.x0_of(), C.X0_CASE.nb_steps
    assert C.M.margin(net, x0, x, h, n) >= C.MIN_MARGIN
    t64, C64, f64 = (a.detach().numpy() for a in C.curve64(copy.deepcopy(net).double(), x0.double(), x.double(), h.double(), n))
    netg, xg, hg, x0g = _on(dev, net, x, h, x0)
    with torch.no_grad():
        t, Cv, f = umnn_amd.IntegralCurve.apply(x0g, xg, netg, None, hg, n)
        F = I.hip_forward_multi(I.mlp_spec(netg), x0g, xg, hg, n)[0]
    errs = [U.rel_err(a.cpu().numpy(), b) for a, b in ((t, t64), (Cv, C64), (f, f64))]
    print(f"x0 != 0: t {errs[0]:.2e} C {errs[1]:.2e} f {errs[2]:.2e}")
    assert I.path_taken() == "hip" and max(errs) <= TOL
    assert torch.equal(t[:, :1], x0g) and torch.equal(t[:, -1:], xg) and torch.equal(Cv[:, 0], torch.zeros_like(Cv[:, 0]))
    assert U.rel_err(Cv[:, -1].cpu().numpy(), F.cpu().numpy()) <= TOL


def test_k17_runs_on_aten_on_the_gpu(dev):
    model, x, h = C.build(C.CASES[4])
    T = C.case_truth(4)
    mg, xg, hg = _on(dev, model, x, h)
    n0 = _count()
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        out = _curve(mg, xg, hg)
        with torch.no_grad():
            cif = mg.cumulative_incidence(xg, hg, curve=True)[1]
    assert _count() == n0 and I.path_taken() == "aten"
    assert max(_errs(out, T)) <= TOL and cif.shape == (33, 21, 17)


# ------------------------------------------------------------------------------------------------------------ identity
def test_two_runs_are_bit_identical_and_precision_settings_do_not_matter(dev):
    for i in (1, 3):
        model, x, h = C.build(C.CASES[i])
        mg, xg, hg = _on(dev, model, x, h)
        ref = _curve(mg, xg, hg)
        with torch.no_grad():
            ref_cif = mg.cumulative_incidence(xg, hg)
        for name in (None, "fp32", "bf16x3", "bf16x6", "f16x3"):
            if name is not None:
                umnn_amd.set_precision(name)
            for a, b in zip(_curve(mg, xg, hg), ref):
                assert torch.equal(a, b), (i, name)
            with torch.no_grad():
                assert torch.equal(mg.cumulative_incidence(xg, hg), ref_cif), (i, name)


def test_half_precision_callers_are_converted_at_the_boundary(dev):
    model, x, h = C.build(C.CASES[1])
    mg, xg, hg = _on(dev, model, x, h)
    with torch.no_grad():
        t, Cv, f = umnn_amd.IntegralCurve.apply(None, xg.bfloat16(), mg.integrand, None, hg.bfloat16(), 20)
        t32, C32, f32 = umnn_amd.IntegralCurve.apply(None, xg.bfloat16().float(), mg.integrand, None, hg.bfloat16().float(), 20)
    assert I.path_taken() == "hip" and Cv.dtype == f.dtype == torch.bfloat16
    assert torch.equal(Cv, C32.bfloat16()) and torch.equal(f, f32.bfloat16())


# ------------------------------------------------------------------------------------------------------------ gradients
def test_requires_grad_takes_the_aten_path_and_matches_float64(dev):
    i = 1
    model, x, h = C.build(C.CASES[i])
    T = C.case_truth(i)
    mg, xg, hg = _on(dev, model, x, h)
    xr, hr = xg.clone().requires_grad_(), hg.clone().requires_grad_()
    for p in mg.parameters():
        p.requires_grad_(False)
    n0 = _count()
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        t, y = mg.forward_curve(xr, hr)
    assert I.path_taken() == "aten" and _count() == n0 and y.requires_grad
    (y * T.G.float().to(dev)).sum().backward()
    ex, eh = U.scaled_err(xr.grad.cpu().numpy(), T.dx), U.scaled_err(hr.grad.cpu().numpy(), T.dh)
    print(f"ATen under autograd: dx {ex:.2e} dh {eh:.2e}")
    assert ex <= TOL and eh <= TOL
    # nothing requires grad (frozen parameters, plain inputs): the kernels, also with grad mode on
    t, y = mg.forward_curve(xg, hg)
    assert I.path_taken() == "hip" and not y.requires_grad
    # trainable parameters count as an input that requires grad
    for p in mg.parameters():
        p.requires_grad_(True)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        t, y = mg.forward_curve(xg, hg)
        cif = mg.cumulative_incidence(xg, hg)
    assert I.path_taken() == "aten" and y.requires_grad and cif.requires_grad
    cif.sum().backward()
    assert all(p.grad is not None for p in mg.parameters())


# ------------------------------------------------------------------------------------------------------------ graph mode
class _Curve(torch.nn.Module):
    def __init__(self, m):
        super().__init__()
        self.m = m

    def forward(self, x, h):
        with torch.no_grad():
            return self.m.forward_curve(x, h, with_derivative=True)


def test_compile_and_export_record_the_two_ops_and_reproduce_eager(dev):
    _, x, h = C.build(C.CASES[1])
    torch.manual_seed(3)
    model = umnn_amd.MonotonicNN(3, [20, 33, 17], nb_steps=20, n_out=5)          # (the package's own integrand class, as a user compiles it)
    mg, xg, hg = _on(dev, model, x, h)
    wrap = _Curve(mg).eval()
    eager = wrap(xg, hg)
    assert I.path_taken() == "hip"
    torch._dynamo.reset()
    n0 = _count()
    compiled = torch.compile(wrap, fullgraph=True, backend="aot_eager")(xg, hg)
    torch._dynamo.reset()
    assert _count() - n0 == 2 and _kname().startswith("cc_cumulate")
    for a, b in zip(eager, compiled):
        assert a.shape == b.shape and torch.equal(a, b)
    ep = torch.export.export(wrap, (xg, hg))
    # (the no_grad regions are sub-graphs of the exported program: the ops sit inside them)
    text = "\n".join(str(gm.graph) for gm in ep.graph_module.modules() if isinstance(gm, torch.fx.GraphModule))
    assert "umnn.cc_forward_multi_nodes" in text and "umnn.cc_cumulate" in text
    for a, b in zip(eager, ep.module()(xg, hg)):
        assert torch.equal(a, b)


def test_hipgraph_capture_and_replay_match_eager(dev):
    model, x, h = C.build(C.CASES[3])
    mg, xg, hg = _on(dev, model, x, h)
    with torch.no_grad():
        xs = xg.clone()
        side = torch.cuda.Stream(device=dev)
        side.wait_stream(torch.cuda.current_stream(dev))
        with torch.cuda.stream(side):
            mg.cumulative_incidence(xs, hg, curve=True)                    # (tables uploaded, LDS attributes set)
        torch.cuda.current_stream(dev).wait_stream(side)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            cap = mg.forward_curve(xs, hg, with_derivative=True) + mg.cumulative_incidence(xs, hg, curve=True)[1:]
        xs.copy_(xg * 0.5)
        graph.replay()
        ref = mg.forward_curve(xs, hg, with_derivative=True) + mg.cumulative_incidence(xs, hg, curve=True)[1:]
    torch.cuda.synchronize()
    for a, b in zip(cap, ref):
        assert torch.equal(a, b)
