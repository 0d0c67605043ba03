"""The adjoint-sweep kernel (umnn_flow_adjoint_update) and the gradient through a flow sample on the device.

Truth: tests/_flow_inverse_truth.py -- the float64 oracle's inverse, the dense per-sample Jacobian of the ``.double()`` model's forward,
lam* = solve(J^T, g_x), g_theta* = autograd.grad(forward(x64), params, -lam*) --, built once per case on the CPU and shared.

Bounds.  The kernel: 8 2^-24 (|lam| + |(g - r) e^-lj|) per entry against the formula in float64 on the same fp32 inputs -- one rounding
per operation plus a 2-ulp exp.  The gradients: max |a - b| / max |b| <= 1e-4 kappa, where 1e-4 is what tests/test_gpu_backward.py holds
the same backward kernels to and kappa = max_b ||J_b^-T||_inf ||J_b^T||_inf comes from the float64 J: the first-order perturbation
bound of a linear solve whose matrix is known to 1e-4.  The seeds are chosen with kappa <= 50, which every case asserts.
Measured on one MI355X (fraction of the bound, worst gradient of the case; every test prints its own): the kernel 0.11-0.18; the blocks 0.004-0.012
under both backward precisions; the two-block rsample 0.75 (Flow0's second integrand weight, 1.6e-3 of its largest entry; g_z 1.2e-4).  The
last one is not the kernels' arithmetic (the same under fp32 / fp32 and with adj_tol = 0; the plain training backward at the truth's x is
5e-6 off) but the float32 solve's x, 8.5e-6 from x64 after two blocks, meeting LeakyReLU kinks: the parameter gradient is only piecewise
smooth in x, and moving x64 by 1e-5 in FLOAT64 changes the dense-solve truth itself by up to 1.6e-3 (EXPERIMENTS.md)."""
import copy

import numpy as np
import pytest
import torch

import umnn_amd
from tests import _flow_inverse_truth as FT
from tests import _util as U
from umnn_amd import _lib, integral as I

pytestmark = pytest.mark.gpu
TOL = 1e-4


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


# ---- 1. the kernel --------------------------------------------------------------------------------------------------------------
def _operands(B, d, dev):
    """g, r, log_jac, lam [B,d] fp32: r within 1e-7 max(1, |g|) of g (converged under tol = 1e-6), D = e^lj over two decades."""
    gen = torch.Generator().manual_seed(B * d)
    g = 2. * torch.randn(B, d, generator=gen)
    r = g - 1e-7 * g.abs().clamp(min=1.) * (2. * torch.rand(B, d, generator=gen) - 1.)
    lj = 2.3 * (2. * torch.rand(B, d, generator=gen) - 1.)
    lam = torch.randn(B, d, generator=gen)
    return [t.to(dev) for t in (g, r, lj, lam)]


def _run(g, r, lj, lam, tol, out=None):
    flags = torch.zeros(1, dtype=torch.int32, device=g.device)
    out = I.flow_adjoint_update(g, r, lj, lam, tol, flags, out=out)
    return out, int(flags.item())


def _check_formula(out, g, r, lj, lam, tag):
    g64, r64, lj64, lam64 = (t.double().cpu() for t in (g, r, lj, lam))
    term = (g64 - r64) * torch.exp(-lj64)
    bound = 8 * 2. ** -24 * (lam64.abs() + term.abs())
    err = (out.double().cpu() - (lam64 + term)).abs()
    ok = torch.isfinite(term)
    frac = float((err[ok] / bound[ok]).max())
    print(f"{tag}: worst error {frac:.3f} of the bound 8 2^-24 (|lam| + |term|)")
    assert frac <= 1.


@pytest.mark.parametrize("B,d", [(5, 7), (37, 7)], ids=["35-partial-wave", "259-second-workgroup"])
def test_update_kernel(B, d, dev):
    g, r, lj, lam = _operands(B, d, dev)
    last = (B - 1, d - 1)                        # the last lane of the last (partial) wave
    # converged everywhere: the formula, no bit
    out, word = _run(g, r, lj, lam, 1e-6)
    assert word == 0 and out.data_ptr() != lam.data_ptr()
    _check_formula(out, g, r, lj, lam, f"B d = {B * d}, converged")
    # a residual of order one: the formula again (no cancellation in g - r)
    r_far = (r + torch.randn(B, d, generator=torch.Generator().manual_seed(1)).to(dev)).contiguous()
    out_far, word = _run(g, r_far, lj, lam, 1e-6)
    assert word == 1
    _check_formula(out_far, g, r_far, lj, lam, f"B d = {B * d}, far")
    # lam_out aliasing lam: the same bits
    buf = lam.clone()
    out_alias, word = _run(g, r_far, lj, buf, 1e-6, out=buf)
    assert out_alias is buf and word == 1 and torch.equal(buf, out_far)
    # one entry over tol -- in the last lane, and alone in the first wave
    for b, i in (last, (0, 0)):
        r_one = r.clone()
        r_one[b, i] = g[b, i] - 3e-6 * max(1., abs(float(g[b, i])))
        assert _run(g, r_one, lj, lam, 1e-6)[1] == 1, (b, i)
        r_one[b, i] = g[b, i] - 0.5e-6 * max(1., abs(float(g[b, i])))
        assert _run(g, r_one, lj, lam, 1e-6)[1] == 0, (b, i)
    # tol = 0: any non-zero residual sets bit 0, an exact one does not
    assert _run(g, r, lj, lam, 0.)[1] == 1
    assert _run(g, g.clone(), lj, lam, 0.)[1] == 0
    # one NaN entry: bit 1 only -- it never counts as "not converged" --, that entry NaN, every other entry the clean launch's bits
    for b, i in (last, (1, 3)):
        r_nan = r.clone()
        r_nan[b, i] = float("nan")
        out_nan, word = _run(g, r_nan, lj, lam, 1e-6)
        assert word == 2, (b, i)
        clean = torch.ones(B, d, dtype=torch.bool, device=dev)
        clean[b, i] = False
        assert torch.isnan(out_nan[b, i]) and torch.equal(out_nan[clean], out[clean])
    g_inf = g.clone()
    g_inf[0, 1] = float("inf")
    assert _run(g_inf, r, lj, lam, 1e-6)[1] == 2
    r_both = r.clone()
    r_both[last] = g[last] - 1.
    r_both[0, 2] = float("nan")
    assert _run(g, r_both, lj, lam, 1e-6)[1] == 3
    # flags are ORed into, not overwritten
    flags = torch.full((1,), 4, dtype=torch.int32, device=dev)
    I.flow_adjoint_update(g, r_far, lj, lam, 1e-6, flags)
    assert int(flags.item()) == 5


def test_update_kernel_empty_batch(dev):
    e = torch.empty(0, 7, device=dev)
    before = _lib.lib().umnn_launch_count()
    out, word = _run(e, e, e, e, 1e-6)
    assert out.shape == (0, 7) and word == 0 and _lib.lib().umnn_launch_count() == before


# ---- 2. one block: the three families of the backward, both backward precisions -----------------------------------------------------
B_BLK, D_BLK, N_BLK = 5, 7, 20                  # 35 rows = three tiles, every tile straddling samples
NETS = [([50] * 4, 30, 3), ([100, 50, 50, 50, 50], 30, 5), ([40, 33], 3, 4)]       # (hidden, E, seed: chosen for kappa <= 50)
_CASES = {}


def _block_case(hid, E, seed):
    key = (tuple(hid), E)
    if key not in _CASES:
        m = FT.make_flow(D_BLK, hid, E, N_BLK, 1, seed=seed, made_hidden=(64, 64), made_gain=3.)
        gen = torch.Generator().manual_seed(seed + 100)
        x0 = 1.5 * torch.randn(B_BLK, D_BLK, generator=gen, dtype=torch.float64)
        G = torch.randn(B_BLK, D_BLK, generator=gen)
        with torch.no_grad():
            z = FT.double_of(m).nets[0](x0).float()
        tr = FT.truth(m, z.double(), lambda x: G.double(), module=m.nets[0])
        _CASES[key] = (m, z, G, tr)
    return _CASES[key]


def _compare(tag, tr, kappa, got):
    """``got``: {name: tensor}, "g_z" among them -> worst fraction of the bound 1e-4 kappa."""
    bound = TOL * kappa
    errs = {}
    for k, v in got.items():
        ref = tr.lam if k == "g_z" else tr.grads[k]
        errs[k] = U.scaled_err(v.detach().cpu().numpy(), ref.numpy())
    worst = max(errs, key=errs.get)
    print(f"{tag}: kappa {kappa:.1f}, bound {bound:.2e}; g_z {errs['g_z'] / bound:.3f} of it, worst {worst} {errs[worst] / bound:.3f} of it")
    assert all(e <= bound for e in errs.values()), {k: e / bound for k, e in errs.items()}


@pytest.mark.parametrize("precision", ["bf16x3", "fp32"])
@pytest.mark.parametrize("hid,E,seed", NETS, ids=["x".join(map(str, n[0])) for n in NETS])
def test_block_gradients(hid, E, seed, precision, dev):
    m_cpu, z, G, tr = _block_case(hid, E, seed)
    assert tr.kappa <= 50., tr.kappa
    umnn_amd.set_backward_precision(precision)
    blk = copy.deepcopy(m_cpu).to(dev).nets[0]
    umnn_amd.invalidate_caches(blk)
    zz = z.to(dev).requires_grad_()
    x, info = blk.inverse(zz, return_info=True)
    assert umnn_amd.path_taken() == "hip"
    assert float((x.detach().cpu().double() - tr.x).abs().max()) <= TOL / min(tr.min_sf)
    params = {k: p for k, p in blk.named_parameters() if p.requires_grad}
    assert "scaling" not in params and len(params) == 6 + 2 * (len(hid) + 1)
    launches = _lib.lib().umnn_launch_count()
    out = torch.autograd.grad((x * G.to(dev)).sum(), [zz] + list(params.values()))
    torch.cuda.synchronize()
    assert umnn_amd.backward_path_taken() == "hip" and _lib.lib().umnn_launch_count() > launches
    rec = info["adjoint"][0]
    print(f"{hid} {precision}: adjoint {rec}, backward kernel {_lib.lib().umnn_last_kernel_name_of(_lib.PROF_BACKWARD).decode()}")
    assert 1 <= rec["vjps"] <= D_BLK and rec["sweeps"] <= D_BLK and not rec["flags"] & 2
    _compare(f"{hid} {precision}", tr, tr.kappa, dict(zip(["g_z"] + list(params), out)))
    # the module is as it was: flags of the parameters, no .grad written by the sweeps
    assert all(p.grad is None for p in blk.parameters()) and not blk.scaling.requires_grad


def test_block_exact_sweeps_and_jacobi_solve(dev):
    """adj_tol = 0: exactly d sweeps and no flag read; the Jacobi solve in front of the same adjoint: the same bound."""
    hid, E, seed = NETS[0]
    m_cpu, z, G, tr = _block_case(hid, E, seed)
    blk = copy.deepcopy(m_cpu).to(dev).nets[0]
    umnn_amd.invalidate_caches(blk)
    params = {k: p for k, p in blk.named_parameters() if p.requires_grad}
    for kw in (dict(adj_tol=0.), dict(method="jacobi")):
        zz = z.to(dev).requires_grad_()
        x, info = blk.inverse(zz, return_info=True, **kw)
        out = torch.autograd.grad((x * G.to(dev)).sum(), [zz] + list(params.values()))
        assert umnn_amd.backward_path_taken() == "hip"
        rec = info["adjoint"][0]
        if "adj_tol" in kw:
            assert rec == {"sweeps": D_BLK, "vjps": D_BLK, "flags": None}
        else:
            assert info["solve"][0]["sweeps"] <= D_BLK and rec["vjps"] <= D_BLK
        _compare(f"{hid} {kw}", tr, tr.kappa, dict(zip(["g_z"] + list(params), out)))


# ---- 3. end to end: rsample of a two-block flow --------------------------------------------------------------------------------------
def test_rsample_end_to_end(dev):
    d, B, n, seed = 6, 33, 20, 2
    m_cpu = FT.make_flow(d, [50] * 4, 30, n, 2, seed=seed, made_hidden=(64, 64), made_gain=2.)
    z = torch.randn(B, d, generator=torch.Generator().manual_seed(11))             # what rsample draws from this generator
    tr = FT.truth(m_cpu, z.double(), lambda x: 2. * x)
    kappa = float(np.prod(tr.block_kappas))
    assert all(k <= 50. for k in tr.block_kappas), tr.block_kappas
    m = copy.deepcopy(m_cpu).to(dev)
    umnn_amd.invalidate_caches(m)
    x, info = m.rsample(B, generator=torch.Generator().manual_seed(11), return_info=True)
    assert x.is_cuda and x.requires_grad and umnn_amd.path_taken() == "hip"
    assert float((x.detach().cpu().double() - tr.x).abs().max()) <= sum(TOL / v for v in tr.min_sf)
    params = {k: p for k, p in m.named_parameters() if p.requires_grad}
    out = torch.autograd.grad(x.square().sum(), list(params.values()))
    torch.cuda.synchronize()
    assert umnn_amd.backward_path_taken() == "hip"
    print(f"rsample: adjoint {info['adjoint']}, block kappas {tr.block_kappas}")
    assert len(info["adjoint"]) == 2 and all(1 <= rec["vjps"] <= d and rec["sweeps"] <= d and not rec["flags"] & 2 for rec in info["adjoint"])
    bound = TOL * kappa
    errs = {k: U.scaled_err(v.cpu().numpy(), tr.grads[k].numpy()) for k, v in zip(params, out)}
    worst = max(errs, key=errs.get)
    print(f"rsample: kappa (product over the blocks) {kappa:.1f}, bound {bound:.2e}, worst {worst} {errs[worst] / bound:.3f} of it")
    assert all(e <= bound for e in errs.values()), {k: e / bound for k, e in errs.items()}
    # sample: the same draw without a graph; log_prob: compute_ll's first output
    s = m.sample(B, generator=torch.Generator().manual_seed(11))
    assert torch.equal(s, x.detach()) and not s.requires_grad
    with torch.no_grad():
        assert torch.equal(m.log_prob(s), m.compute_ll(s)[0])
