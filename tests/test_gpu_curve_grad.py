"""Training through the curves on the GPU: ``forward_curve`` / ``cumulative_incidence`` / ``IntegralCurve`` / ``cumulate`` with
``backward="hip"`` (csrc/cc_multi.hip: the node-cotangent builds of cc_bwd_multi_kernel; csrc/cc_cumulate.hip: the adjoint build)
against the float64 truth on every kernel family, a non-zero lower limit, a ragged last group, the nested integral, bit-identity,
``need`` handling, the ATen fallbacks and graph mode.  Cases, truth, tolerance (1e-5 per tensor) and kink margins:
tests/_curve_grad_cases.py."""
import copy
import warnings

import numpy as np
import pytest
import torch

import umnn_amd
from tests import _curve_cases as C
from tests import _curve_grad_cases as G
from tests import _util as U
from umnn_amd import _lib, integral as I, nets

pytestmark = pytest.mark.gpu
TOL = G.TOL


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


def _count():
    return _lib.lib().umnn_launch_count()


def _kname():
    """The calling thread's last kernel: the forward's."""
    return _lib.lib().umnn_last_kernel_name().decode()


def _bname():
    """The last backward pass of the process (backward runs on autograd's worker threads)."""
    return _lib.lib().umnn_last_kernel_name_of(_lib.PROF_BACKWARD).decode()


def _on(dev, model, *tensors):
    return (copy.deepcopy(model).to(dev),) + tuple(t.to(dev) for t in tensors)


def _model_grads(mg, xg, hg, Gd, backward="hip", need_x=True, need_h=True):
    """-> (outputs, [dx, dh, {parameter: grad}], launches of the forward, launches of the backward)."""
    mg.zero_grad()
    xr = xg.clone().requires_grad_() if need_x else xg
    hr = hg.clone().requires_grad_() if need_h else hg
    n0 = _count()
    out = mg.forward_curve(xr, hr, with_derivative=True, backward=backward)
    n1 = _count()
    G.loss_of(out, Gd).backward()
    torch.cuda.synchronize()
    n2 = _count()
    grads = {k: (None if p.grad is None else p.grad.clone()) for k, p in mg.named_parameters()}
    return out, [xr.grad, hr.grad, grads], n1 - n0, n2 - n1


def _check(tag, got, T):
    dx, dh, dparams = got
    errs = {"dx": U.scaled_err(dx.cpu().numpy(), T.dx), "dh": U.scaled_err(dh.cpu().numpy(), T.dh)}
    for k, v in dparams.items():
        errs[k] = U.scaled_err(v.cpu().numpy(), T.dparams[k])
    worst = max(v for k, v in errs.items() if k not in ("dx", "dh"))
    print(f"{tag}: dx {errs['dx']:.2e} dh {errs['dh']:.2e} worst parameter {worst:.2e}")
    assert set(dparams) == set(T.dparams)
    for k, v in errs.items():
        assert v <= TOL, (k, v)


# ------------------------------------------------------------------------------------------------------------ 1. every family
@pytest.mark.parametrize("i", G.HIP_CASES)
def test_forward_curve_hip_backward_matches_float64(dev, i):
    model, x, h = G.build(i)
    T = G.case_truth(i)
    print(f"case {i}: margin {T.margin:.2e}")
    assert T.margin >= G.MIN_MARGIN and float(x[0]) == 0.
    mg, xg, hg = _on(dev, model, x, h)
    Gd = G.on(G.cotangents(x.shape[0], model.nb_steps, model.n_out), xg)
    with torch.no_grad():
        ref = mg.forward_curve(xg, hg, with_derivative=True)
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        out, got, n_fwd, n_bwd = _model_grads(mg, xg, hg, Gd)
    assert n_fwd == 2 and n_bwd >= 2 and I.backward_path_taken() == "hip" and "NC=1" in _bname()
    for a, b in zip(out, ref):
        assert a.requires_grad and torch.equal(a.detach(), b)
    _check(f"case {i}", got, T)


# ------------------------------------------------------------------------------------------------------------ 2. the operator, x0 != 0
def test_operator_with_nonzero_x0(dev):
    net, x0, x, h, n = G.x0_case()
    T = G.x0_truth()
    print(f"x0 != 0: margin {T.margin:.2e}")
    assert T.margin >= G.MIN_MARGIN and bool((x[0] == x0[0]).all())
    netg, x0g, xg, hg = _on(dev, net, x0, x, h)
    Gd = G.on(G.cotangents(x.shape[0], n, C.X0_CASE.K), xg)
    with torch.no_grad():
        ref = umnn_amd.IntegralCurve.apply(x0g, xg, netg, None, hg, n)
    x0r, xr, hr = (v.clone().requires_grad_() for v in (x0g, xg, hg))
    flat = I._flatten(netg.parameters())
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        out = umnn_amd.IntegralCurve.apply(x0r, xr, netg, flat, hr, n, backward="hip")
        for a, b in zip(out, ref):
            assert torch.equal(a.detach(), b)
        G.loss_of(out, Gd).backward()
    assert I.backward_path_taken() == "hip"
    e0 = U.scaled_err(x0r.grad.cpu().numpy(), T.dx0)
    print(f"x0 != 0: dx0 {e0:.2e}")
    assert e0 <= TOL
    _check("x0 != 0", [xr.grad, hr.grad, {k: p.grad for k, p in netg.named_parameters()}], T)


# ------------------------------------------------------------------------------------------------------------ 3. ragged last group
def test_ragged_last_group_and_more_groups_than_waves(dev):
    cus = torch.cuda.get_device_properties(dev).multi_processor_count
    model, x, h, idx, G64 = G.ragged_case(cus)
    B0 = C.P2_BASE.B
    assert x.shape[0] == cus * 4 * 16 + 5
    T = G.model_truth(model, x, h, G64)                        # the float64 truth of the repeated batch
    base = G.model_truth(model, x[:B0], h[:B0], tuple(g[:B0] for g in G64))
    print(f"ragged, B = {x.shape[0]}: margin {base.margin:.2e}")
    assert base.margin >= G.MIN_MARGIN
    mg, xg, hg = _on(dev, model, x, h)
    out, (dx, dh, dparams), _, _ = _model_grads(mg, xg, hg, G.on(G64, xg))
    assert I.backward_path_taken() == "hip"
    # per row against the base rows' truth; every copy of a base row has that row's bits
    ex, eh = U.scaled_err(dx.cpu().numpy(), base.dx[idx.numpy()]), U.scaled_err(dh.cpu().numpy(), base.dh[idx.numpy()])
    print(f"ragged: dx {ex:.2e} dh {eh:.2e} (per row, against the base rows)")
    assert ex <= TOL and eh <= TOL
    assert torch.equal(dx, dx[:B0][idx.to(dev)])
    _check("ragged, whole batch", [dx, dh, dparams], T)


# ------------------------------------------------------------------------------------------------------------ 4. the nested integral
def test_cumulative_incidence_hip_backward_matches_float64(dev):
    model, x, h = G.cif_case()
    G64, dh64, dparams64 = G.cif_truth()
    mg, xg, hg = _on(dev, model, x, h)
    with torch.no_grad():
        ref = mg.cumulative_incidence(xg, hg, curve=True)[1]
    hr = hg.clone().requires_grad_()
    n0 = _count()
    cif = mg.cumulative_incidence(xg, hr, curve=True, backward="hip")[1]
    assert _count() - n0 == 3 and _kname() == "cc_cumulate<MT=4>" and I.path_taken() == "hip"      # cumulate ran its kernel
    assert torch.equal(cif.detach(), ref)
    n1 = _count()
    (cif * G64.float().to(dev)).sum().backward()
    torch.cuda.synchronize()
    assert I.backward_path_taken() == "hip" and _count() - n1 >= 3          # two adjoint launches and the backward's passes
    errs = {"dh": U.scaled_err(hr.grad.cpu().numpy(), dh64)}
    for k, p in mg.named_parameters():
        errs[k] = U.scaled_err(p.grad.cpu().numpy(), dparams64[k])
    print("CIF: " + " ".join(f"{k} {v:.2e}" for k, v in errs.items()))
    for k, v in errs.items():
        assert v <= TOL, (k, v)


def test_cumulate_hip_backward_runs_the_adjoint_kernel(dev):
    n, B, K = 20, 37, 5
    g = torch.Generator().manual_seed(2)
    v, x0, x, gC = (torch.randn(s, generator=g) for s in ((B, n + 1, K), (B, 1), (B, 1), (B, n + 1, K)))
    leaves64 = [t.double().clone().requires_grad_() for t in (v, x0, x)]
    want = torch.autograd.grad((I.aten_cumulate(*leaves64, n) * gC.double()).sum(), leaves64)
    leaves = [t.to(dev).requires_grad_() for t in (v, x0, x)]
    with torch.no_grad():
        ref = umnn_amd.integral.cumulate(leaves[0], leaves[1], leaves[2], n)
    n0 = _count()
    out = umnn_amd.integral.cumulate(*leaves, n, backward="hip")
    assert _count() - n0 == 1 and _kname() == "cc_cumulate<MT=2>" and torch.equal(out.detach(), ref)
    got = torch.autograd.grad((out * gC.to(dev)).sum(), leaves)
    torch.cuda.synchronize()
    assert _count() - n0 == 2 and _bname() == "cc_bwd_cumulate_adjoint<MT=2>"
    for name, a, b in zip(("d values", "dx0", "dx"), got, want):
        e = U.scaled_err(a.cpu().numpy(), b.numpy())
        print(f"cumulate: {name} {e:.2e}")
        assert e <= TOL


# ------------------------------------------------------------------------------------------------------------ 5. identity
def test_two_runs_are_bit_identical_and_precision_settings_do_not_matter(dev):
    for i in (1, 2):
        model, x, h = G.build(i)
        mg, xg, hg = _on(dev, model, x, h)
        Gd = G.on(G.cotangents(x.shape[0], model.nb_steps, model.n_out), xg)
        _, ref, _, _ = _model_grads(mg, xg, hg, Gd)
        for name in (None, "fp32", "bf16x3", "bf16x6", "f16x3"):
            if name is not None:
                umnn_amd.set_precision(name)
            _, got, _, _ = _model_grads(mg, xg, hg, Gd)
            assert torch.equal(got[0], ref[0]) and torch.equal(got[1], ref[1]), (i, name)
            for k in ref[2]:
                assert torch.equal(got[2][k], ref[2][k]), (i, name, k)


# ------------------------------------------------------------------------------------------------------------ 6. need
def test_frozen_parameters_launch_only_the_edge_pass_and_unneeded_inputs_get_none(dev):
    i = 2                                                      # hidden [100, 100, 100]: seven tiles, two passes when d_theta is asked for
    model, x, h = G.build(i)
    T = G.case_truth(i)
    mg, xg, hg = _on(dev, model, x, h)
    Gd = G.on(G.cotangents(x.shape[0], model.nb_steps, model.n_out), xg)
    _, full, _, n_full = _model_grads(mg, xg, hg, Gd)
    for p in mg.integrand.parameters():
        p.requires_grad_(False)
    _, frozen, _, n_frozen = _model_grads(mg, xg, hg, Gd)
    print(f"launches of the backward: {n_full} with d_theta, {n_frozen} without")
    assert n_frozen == 2 < n_full                              # the adjoint cumulate and the EDGE pass
    assert "EDGE=1" in _bname() and "NC=1" in _bname()
    assert torch.equal(frozen[0], full[0]) and torch.equal(frozen[1], full[1])
    assert all(frozen[2][k] is None for k in frozen[2] if k.startswith("integrand."))
    for p in mg.integrand.parameters():
        p.requires_grad_(True)
    _, got, _, _ = _model_grads(mg, xg, hg, Gd, need_x=False)
    assert got[0] is None and torch.equal(got[1], full[1])
    # h without grad: the conditioner's parameters still need the curve's cotangents, and x gets its gradient
    netg = mg.integrand
    xr = xg.clone().requires_grad_()
    out = umnn_amd.IntegralCurve.apply(None, xr, netg, I._flatten(netg.parameters()), hg, model.nb_steps, backward="hip")
    G.loss_of(out, Gd).backward()
    assert hg.grad is None and xr.grad is not None and I.backward_path_taken() == "hip"


# ------------------------------------------------------------------------------------------------------------ 7. fallbacks
def _notices(fn):
    with warnings.catch_warnings(record=True) as seen:
        warnings.simplefilter("always")
        out = fn()
    return out, [w for w in seen if issubclass(w.category, RuntimeWarning) and "umnn_amd" in str(w.message)]


def test_k17_and_nb_steps_128_run_aten_with_one_notice_and_correct_gradients(dev):
    model17, x, h = G.build(4)
    assert model17.n_out == 17
    model128, x128, h128 = G.build(1)
    model128.nb_steps = 128
    for tag, what, model, xx, hh, T in (("K = 17", "n_out = 17", model17, x, h, G.case_truth(4)),
                                        ("n = 128", "nb_steps = 128", model128, x128, h128, G.model_truth(model128, x128, h128))):
        assert T.margin >= G.MIN_MARGIN
        mg, xg, hg = _on(dev, model, xx, hh)
        Gd = G.on(G.cotangents(xx.shape[0], model.nb_steps, model.n_out), xg)
        # the notices are given once per process and net: forget the ones an earlier test of these nets has taken
        I._warned.difference_update({k for k in I._warned if isinstance(k, tuple) and k[0] in ("curve-aten", "curve-grad-aten")})
        nets._noticed.discard("wide")
        n0 = _count()
        (_, got, _, _), first = _notices(lambda: _model_grads(mg, xg, hg, Gd))
        _, second = _notices(lambda: _model_grads(mg, xg, hg, Gd))
        print(f"{tag}: {len(first)} notice(s) on the first call, {len(second)} on the second: {[str(w.message) for w in first]}")
        assert _count() == n0 and I.path_taken() == "aten" and I.backward_path_taken() == "aten"
        assert len(first) == 1 and len(second) == 0
        assert "ATen" in str(first[0].message) and what in str(first[0].message)
        _check(tag, got, T)


# ------------------------------------------------------------------------------------------------------------ 8. graph mode
def test_compile_records_the_two_ops_and_reproduces_the_eager_gradients(dev):
    """The loss is compiled (fullgraph, aot_eager) and differentiated with ``torch.autograd.grad``: AOTAutograd traces the backward
    of ``CurveFunction`` into the backward graph.  (``autograd.grad`` itself cannot stand inside a fullgraph region: Dynamo refuses
    to trace it.)  A second compile through a recording AOT backend shows the ops of that backward graph."""
    import torch._dynamo
    from torch._dynamo.backends.common import aot_autograd
    from functorch.compile import make_boxed_func
    _, x, h = G.build(1)
    torch.manual_seed(3)
    model = umnn_amd.MonotonicNN(3, [20, 33, 17], nb_steps=20, n_out=5)          # (the package's own integrand class, as a user compiles it)
    mg, xg, hg = _on(dev, model, x, h)
    Gd = G.on(G.cotangents(x.shape[0], 20, 5), xg)
    params = list(mg.parameters())

    def loss_fn(xx, hh):
        return G.loss_of(mg.forward_curve(xx, hh, with_derivative=True, backward="hip"), Gd)

    def run(fn):
        xr, hr = xg.clone().requires_grad_(), hg.clone().requires_grad_()
        loss = fn(xr, hr)
        return [loss.detach()] + list(torch.autograd.grad(loss, [xr, hr] + params))

    eager = run(loss_fn)
    assert I.backward_path_taken() == "hip"
    torch._dynamo.reset()
    compiled = run(torch.compile(loss_fn, fullgraph=True, backend="aot_eager"))
    assert I.backward_path_taken() == "hip" and "NC=1" in _bname()
    for a, b in zip(eager, compiled):
        assert a.shape == b.shape and torch.equal(a, b)
    torch._dynamo.reset()
    graphs = []

    def record(gm, example_inputs):
        graphs.append(str(gm.graph))
        return make_boxed_func(gm.forward)

    recorded = run(torch.compile(loss_fn, fullgraph=True, backend=aot_autograd(fw_compiler=record, bw_compiler=record)))
    torch._dynamo.reset()
    text = "\n".join(graphs)
    assert "umnn.cc_forward_multi_nodes" in text and "umnn.cc_cumulate" in text
    assert "umnn.cc_cumulate_adjoint" in text and "umnn.cc_backward_multi_nodes" in text
    for a, b in zip(eager, recorded):
        assert torch.equal(a, b)
