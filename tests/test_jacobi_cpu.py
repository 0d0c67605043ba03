"""``invert(method="jacobi")`` and the warm start of ``integral.newton_solve`` without a GPU (the generic ATen path).

Truth and bounds are those of tests/test_inverse_cpu.py: the float64 solve of tests/_inverse_truth.py over the numpy oracle, TOL = 1e-4
the forward parity tolerance, |x_hat - x| <= sum over blocks of TOL / min exp(s) f, m(x_hat) = z to TOL.  Flows are default-initialised;
where more sweeps are wanted the MADE weights are multiplied by 3 (stronger coupling between the dimensions)."""
import copy

import numpy as np
import pytest
import torch

import umnn_amd
from oracle import cc_oracle as O
from tests import _inverse_truth as T
from tests import _util as U
from umnn_amd import integral
from umnn_amd.nets import IntegrandNetwork

TOL = 1e-4
N = 20


def _flow(d, nb_flow, seed, made_gain=1., cond_in=0, E=10):
    torch.manual_seed(seed)
    m = umnn_amd.UMNNMAFFlow(nb_flow=nb_flow, nb_in=d, hidden_derivative=[50] * 4, hidden_embedding=[32, 32], embedding_s=E,
                             nb_steps=N, solver="CCParallel", cond_in=cond_in).eval()
    if made_gain != 1.:
        with torch.no_grad():
            for blk in m.nets:
                for mod in blk.net.made.net:
                    if hasattr(mod, "weight"):
                        mod.weight.mul_(made_gain)
    return m


def _model_bound(m, x, context=None):
    """sum over blocks of TOL / min exp(s) f from the model's own log_jac in float64 (as tests/test_gpu_solve_coverage._flow_bound)."""
    m64 = copy.deepcopy(m).double()
    umnn_amd.invalidate_caches(m64)
    xi = x.double()
    ctx = None if context is None else context.double()
    total = 0.
    with torch.no_grad():
        for blk in m64.nets:
            z, lj = blk._transform(xi, ctx, want_jac=True)
            total += TOL / float(torch.exp(lj.min()))
            xi = torch.flip(z, [1])
    return total


@pytest.mark.parametrize("nb_flow", [1, 2])
def test_flow_against_truth(nb_flow):
    d, B = 8, 16
    m = _flow(d, nb_flow, seed=11 + nb_flow)
    blocks = T.blocks_from_state_dict(m.state_dict(), nb_flow)
    x = 1.5 * np.random.default_rng(nb_flow).standard_normal((B, d))
    z64 = O.flow_forward(blocks, x, N)
    x_true, mins = T.flow_invert64(blocks, z64, N)
    bound = sum(TOL / v for v in mins)
    assert np.max(np.abs(x_true - x)) < 1e-9 and 1e-5 < bound < 1e-2, (mins, bound)
    z = torch.from_numpy(z64.astype(np.float32))
    with torch.no_grad():
        x_hat, info = m.invert(z, method="jacobi", return_info=True)
        assert torch.equal(m.invert(z, method="jacobi"), x_hat)
        z_back = m(x_hat)
    assert umnn_amd.path_taken() == "aten"
    err = float(np.max(np.abs(x_hat.numpy().astype(np.float64) - x_true)))
    res = U.rel_err(z_back.numpy(), z64)
    print(f"jacobi nb_flow={nb_flow}: |x_hat - x| {err:.2e} (bound {bound:.2e}), m(x_hat) vs z {res:.2e}, sweeps {info['sweeps']}, "
          f"evaluations per sweep {info['max_evals']}")
    assert err <= bound
    assert res <= TOL
    assert len(info["sweeps"]) == nb_flow and all(1 <= s <= d for s in info["sweeps"]) and all(info["converged"])
    assert all(len(e) == s for e, s in zip(info["max_evals"], info["sweeps"]))
    assert all(st.shape == (B, d) and st.dtype == torch.int32 for st in info["status"])


def test_one_dimension_takes_one_sweep():
    m = _flow(1, 1, seed=3)
    z = torch.randn(16, 1, generator=torch.Generator().manual_seed(0))
    with torch.no_grad():
        x_hat, info = m.invert(z, method="jacobi", return_info=True)
        x_seq = m.invert(z, method="newton")
    assert info["sweeps"] == [1] and info["converged"] == [True]
    assert torch.equal(x_hat, x_seq)              # (one cold-started solve under the same embedding: the same iteration)


def test_sweep_structure_with_stronger_coupling():
    d, B = 8, 16
    m = _flow(d, 1, seed=5, made_gain=3.)
    x = 1.5 * torch.randn(B, d, generator=torch.Generator().manual_seed(1))
    bound = _model_bound(m, x)
    with torch.no_grad():
        z = m(x)
        x_hat, info = m.invert(z, method="jacobi", return_info=True)
        x_all, info_all = m.invert(z, method="jacobi", sweep_tol=0., return_info=True)
        x_seq = m.invert(z, method="newton")
        x_one, info_one = m.invert(z, method="jacobi", max_sweeps=1, return_info=True)
        blk_x, blk_info = m.nets[0].invert(z, method="jacobi", return_info=True)
    print(f"x3 MADE weights: sweeps {info['sweeps']}, evaluations per sweep {info['max_evals']}, "
          f"|x_hat - x| {float((x_hat - x).abs().max()):.2e}, |x_d - x_seq| {float((x_all - x_seq).abs().max()):.2e} (bound {bound:.2e})")
    assert 2 < info["sweeps"][0] <= d and info["converged"] == [True]
    assert float((x_hat - x).abs().max()) <= bound
    # sweep_tol = 0: exactly d sweeps, the count at which the result is the sequential one by construction
    assert info_all["sweeps"] == [d] and info_all["converged"] == [True]
    assert float((x_all - x_seq).abs().max()) <= bound and float((x_all - x).abs().max()) <= bound
    # one sweep of d > 1 coupled dimensions is not the inverse, and says so
    assert info_one["sweeps"] == [1] and info_one["converged"] == [False]
    assert float((x_one - x).abs().max()) > 100 * bound
    assert float((x_one[:, 0] - x[:, 0]).abs().max()) <= bound            # (dimension 0 reads no other: final after sweep 1)
    # the block's own method returns the block's info unlisted
    assert torch.equal(blk_x, x_hat) and blk_info["sweeps"] == info["sweeps"][0] and blk_info["converged"] is True
    with pytest.raises(ValueError, match="unknown inversion method"):
        m.invert(z, method="gauss-seidel")
    with pytest.raises(ValueError, match="max_sweeps"):
        m.invert(z, method="jacobi", max_sweeps=0)


def test_conditional_flow_honours_the_context():
    d, B, cond = 4, 16, 3
    m = _flow(d, 2, seed=9, made_gain=3., cond_in=cond)
    g = torch.Generator().manual_seed(4)
    x = 1.5 * torch.randn(B, d, generator=g)
    ctx = torch.randn(B, cond, generator=g)
    bound = _model_bound(m, x, ctx)
    with torch.no_grad():
        z = m(x, context=ctx)
        x_hat, info = m.invert(z, method="jacobi", context=ctx, return_info=True)
        x_other = m.invert(z, method="jacobi", context=torch.flip(ctx, [0]))
        z_back = m(x_hat, context=ctx)
    err = float((x_hat - x).abs().max())
    print(f"conditional: |x_hat - x| {err:.2e} (bound {bound:.2e}), sweeps {info['sweeps']}")
    assert err <= bound and U.rel_err(z_back.numpy(), z.numpy()) <= TOL
    assert all(s <= d for s in info["sweeps"]) and all(info["converged"])
    assert float((x_other - x).abs().max()) > 100 * bound, "the context is really read"


def _solve_case(dtype):
    torch.manual_seed(2)
    E, B, d = 6, 12, 3
    net = IntegrandNetwork(d, 1 + E, [50, 50, 50], 1).to(dtype)
    g = torch.Generator().manual_seed(8)
    h = torch.randn(B, E * d, generator=g).to(dtype)
    target = (2. * torch.randn(B, d, generator=g)).to(dtype)

    def eval_fn(x):
        with torch.no_grad():
            return integral.aten_forward(net, torch.zeros_like(x), x, h, N), net(x, h)
    return eval_fn, target


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_newton_solve_without_x_init_is_unchanged(dtype):
    """``x_init=None`` is the iteration as it was -- and a start value of 0 is that same iteration."""
    eval_fn, target = _solve_case(dtype)
    ref = integral.newton_solve(eval_fn, target, 1.3, 0.2, -50., 50., 1e-6, 64)
    for out in (integral.newton_solve(eval_fn, target, 1.3, 0.2, -50., 50., 1e-6, 64, x_init=None),
                integral.newton_solve(eval_fn, target, 1.3, 0.2, -50., 50., 1e-6, 64, x_init=torch.zeros_like(target))):
        assert all(torch.equal(a, b) for a, b in zip(out, ref))
    evals = (ref[2] & umnn_amd.SOLVE_EVALS_MASK)
    assert int(evals.min()) >= 2 and int(ref[2].max()) <= umnn_amd.SOLVE_EVALS_MASK       # (no flag; a cold start needs more than one)


def test_newton_solve_warm_start():
    """Started on a converged solution every row stops at its first evaluation and x comes back as given (float64: every row of the
    first solve ended on the residual rule).  Start values outside [lo, hi] are clamped, non-finite ones replaced by 0."""
    eval_fn, target = _solve_case(torch.float64)
    x, fx, status = integral.newton_solve(eval_fn, target, 1.3, 0.2, -50., 50., 1e-6, 64)
    x2, fx2, status2 = integral.newton_solve(eval_fn, target, 1.3, 0.2, -50., 50., 1e-6, 64, x_init=x)
    assert torch.equal(status2, torch.ones_like(status2)), "one evaluation, no flag"
    assert torch.equal(x2, x) and torch.equal(fx2, fx)
    # near the solution: fewer evaluations than cold, the same answer to the tolerance
    x3, _, status3 = integral.newton_solve(eval_fn, target, 1.3, 0.2, -50., 50., 1e-6, 64, x_init=x + 1e-3)
    assert int(status3.max()) <= 2 and float((x3 - x).abs().max()) < 1e-5
    # clamping and non-finite entries, seen through max_iter = 1 (the start point is what leaves)
    start = torch.zeros_like(target)
    start[0, 0], start[1, 0], start[2, 0], start[3, 0], start[4, 0] = 80., -80., float("nan"), float("inf"), 0.7
    x4, _, _ = integral.newton_solve(eval_fn, target, 1.3, 0.2, -5., 6., 1e-6, 1, x_init=start)
    assert x4[:5, 0].tolist() == [6., -5., 0., 0., 0.7] and torch.all(x4[5:] == 0.)


def test_block_entry_point_validates_without_a_gpu():
    import ctypes
    from umnn_amd import _lib
    lib = _lib.lib()
    p = ctypes.c_void_p(0x1000)
    desc = _lib.MlpDesc()
    desc.n_linear = 3
    for i, w in enumerate([3, 16, 16, 1]):
        desc.widths[i] = w
    for l in range(3):
        desc.W[l], desc.b[l] = 0x1000, 0x1000

    def call(B=4, d=3, lo=-50., hi=50., max_iter=64, nb_steps=20, x=p):
        return lib.umnn_cc_solve_block(ctypes.byref(desc), p, p, None, 1, None, p, p, nb_steps, B, d, 2, lo, hi, 1e-6, max_iter,
                                       x, None, None, None)
    assert call(B=0) == 0                                 # an empty batch is a no-op and touches no device
    assert call(d=0) == _lib.EINVAL and call(lo=1., hi=1.) == _lib.EINVAL and call(max_iter=0) == _lib.EINVAL
    assert call(nb_steps=0) == _lib.EINVAL and call(x=None) == _lib.EINVAL and call(B=-1) == _lib.EINVAL
