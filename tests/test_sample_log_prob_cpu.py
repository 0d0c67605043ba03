"""``invert(..., return_log_jac=True)`` and ``sample_and_log_prob`` without a GPU: float64 flows on the generic ATen path.

The log-density of a drawn sample is built from the f(x) the solves already hold.  Against ``compute_ll`` at the returned x it differs by
the solve residual only (the Gaussian term uses the drawn z, ``compute_ll`` the image T(x)): at most d |z| tol times the blocks' O(1) slopes,
about 1e-10 at tol = 1e-12, so the bound 1e-8 max(1, |ll|) leaves two orders of margin.  "jacobi" runs d sweeps with no stop test, where
its result is the sequential one by construction; "bracket" evaluates f at its own (coarser, fp32) x, and is compared at that x."""
import pytest
import torch

import umnn_amd  # noqa: F401
from tests import _sample_log_prob_cases as C

B = C.B
FLOWS, METHODS, _flow, _opts = C.FLOWS, C.METHODS, C.flow, C.opts


@pytest.mark.parametrize("method", list(METHODS))
@pytest.mark.parametrize("name", [f[0] for f in FLOWS])
def test_log_jac_of_invert_matches_compute_ll(name, method):
    m, z, ctx = _flow(name)
    o = _opts(method, z.shape[1])
    x0 = m.invert(z, context=ctx, **o)
    x, lj = m.invert(z, context=ctx, return_log_jac=True, **o)
    assert torch.equal(x, x0), "the flag must not change x"
    assert lj.shape == (B,) and lj.dtype == torch.float64
    with torch.no_grad():
        ll = m.compute_ll(x.double(), ctx)[0]
    log_prob = lj - .5 * (torch.log(m.pi * 2) + z ** 2).sum(1)        # (compute_ll's constant: the flow's pi buffer)
    if method == "bracket":
        # the search's x is no solution to 1e-12: T(x) is not z, so only the Jacobian term is comparable at this x
        with torch.no_grad():
            ref = m.compute_log_jac(x.double(), ctx).sum(1)
        err = (lj - ref).abs() / ref.abs().clamp(min=1.)
    else:
        err = (log_prob - ll).abs() / ll.abs().clamp(min=1.)
    print(f"{name} {method}: max err {float(err.max()):.3e}")
    assert float(err.max()) <= 1e-8


@pytest.mark.parametrize("method", list(METHODS))
def test_single_block_and_triple(method):
    m, z, ctx = _flow("f1-d3")
    blk = m.nets[0]
    o = _opts(method, 3)
    x0 = blk.invert(z, **o)
    x, lj = blk.invert(z, return_log_jac=True, **o)
    assert torch.equal(x, x0)
    with torch.no_grad():
        ref = blk.compute_log_jac(x.double()).sum(1)
    assert float(((lj - ref).abs() / ref.abs().clamp(min=1.)).max()) <= 1e-8
    if o["method"] == "jacobi":
        for obj in (blk, m):
            xi, info, lji = obj.invert(z, return_info=True, return_log_jac=True, **o)
            x2, info2 = obj.invert(z, return_info=True, **o)
            assert torch.equal(xi, x2) and set(info) == set(info2) and info["sweeps"] == info2["sweeps"]
            assert torch.equal(lji, obj.invert(z, return_log_jac=True, **o)[1])
    else:
        with pytest.raises(ValueError):
            blk.invert(z, return_info=True, return_log_jac=True, **o)


@pytest.mark.parametrize("method", list(METHODS))
@pytest.mark.parametrize("name", ["f2-d3", "cond"])
def test_empty_batch(name, method):
    m, z, ctx = _flow(name)
    o = _opts(method, z.shape[1])
    x, lj = m.invert(z[:0], context=None if ctx is None else ctx[:0], return_log_jac=True, **o)
    assert x.shape == (0, z.shape[1]) and lj.shape == (0,)
    x, lp = m.sample_and_log_prob(0, context=None if ctx is None else ctx[:0], **o)
    assert x.shape == (0, z.shape[1]) and lp.shape == (0,)


@pytest.mark.parametrize("method", list(METHODS))
@pytest.mark.parametrize("name", ["f2-d3", "f3-d5", "cond", "sigmoid"])
def test_sample_and_log_prob_is_sample_with_its_density(name, method):
    m, z, ctx = _flow(name)
    o = _opts(method, z.shape[1])
    x0 = m.sample(B, context=ctx, generator=torch.Generator().manual_seed(7), **o)
    x, lp = m.sample_and_log_prob(B, context=ctx, generator=torch.Generator().manual_seed(7), **o)
    assert torch.equal(x, x0) and lp.shape == (B,) and not lp.requires_grad
    if method != "bracket":
        with torch.no_grad():
            ll = m.log_prob(x, ctx)
        assert float(((lp - ll).abs() / ll.abs().clamp(min=1.)).max()) <= 1e-8


@pytest.mark.parametrize("method", list(METHODS))
@pytest.mark.parametrize("name", ["f1-d3", "f3-d3", "cond"])
def test_one_x_whatever_is_asked_for(name, method):
    m, z, ctx = _flow(name)
    o = _opts(method, z.shape[1])
    C.check_one_x(m, len(m.nets), z, ctx, o)
    C.check_one_x(m.nets[0], None, z, ctx, o)


@pytest.mark.parametrize("method", list(METHODS))
@pytest.mark.parametrize("name", ["f2-d3", "f3-d5", "cond"])
def test_flow_invert_is_the_block_inverts_composed(name, method):
    """x is the blocks' x bit for bit; log_jac is the same terms added in another order (the flow threads one running sum through the
    blocks, the composition adds per-block sums).  Two orders of adding n = nb_flow d terms differ by at most 2 (n - 1) eps sum |terms|
    (recursive summation, each order within (n - 1) eps sum |terms| of the exact sum), with sum |terms| taken from the float64 flow's own
    ``_transform`` at x.  Measured in float64: 0 (jacobi, bracket) to 1.5e-16 sum |terms| (newton), against the bound 1e-15 to 6e-15."""
    m, z, ctx = _flow(name)
    o = _opts(method, z.shape[1])
    x, lj = m.invert(z, context=ctx, return_log_jac=True, **o)
    xc, ljc = C.composed(m, z, ctx, o)
    assert torch.equal(xc, x)
    n = len(m.nets) * z.shape[1]
    mag = C.lj_magnitude(m, x, ctx)
    err = ((lj - ljc).abs() / mag).max()
    print(f"{name} {method}: |lj - composed| / sum |terms| {float(err):.2e}")
    assert lj.dtype == ljc.dtype and float(err) <= 2 * (n - 1) * torch.finfo(lj.dtype).eps


def test_sample_and_log_prob_defaults_and_single_block():
    m, _, _ = _flow("f2-d3")
    x, lp = m.sample_and_log_prob(4, generator=torch.Generator().manual_seed(1))
    assert torch.equal(x, m.sample(4, generator=torch.Generator().manual_seed(1)))       # method "newton" by default, like sample
    with torch.no_grad():
        ll = m.log_prob(x)
    # default tol = 1e-6: the residual of the solve is what separates the two, |z| tol per dimension and block slope
    assert float((lp - ll).abs().max()) <= 1e-4
    blk = m.nets[0]
    xb, lpb = blk.sample_and_log_prob(4, generator=torch.Generator().manual_seed(2), tol=1e-12)
    with torch.no_grad():
        llb = blk.compute_ll(xb)[0]
    assert float((lpb - llb).abs().max()) <= 1e-8
    with pytest.raises(ValueError):
        m.sample_and_log_prob(2, method="jacobi", return_info=True)


def test_nonfinite_row_poisons_only_its_own_sum():
    m, z, _ = _flow("f2-d3")
    zz = z.clone()
    zz[2, 1] = float("nan")
    for method in ("newton", "jacobi"):
        x, lj = m.invert(zz, return_log_jac=True, **_opts(method, 3))
        assert torch.isnan(lj[2]) and torch.isfinite(lj[[0, 1, 3, 4, 5]]).all()


def test_entry_points_validate_their_arguments_without_a_gpu():
    """B = 0 is a no-op; null pointers and a bad ``first`` flag are UMNN_EINVAL with a message (nothing is launched)."""
    import ctypes
    from umnn_amd import _lib
    lib = _lib.lib()
    p = ctypes.c_void_p(0x1000)
    assert lib.umnn_flow_sample_lj_rows(None, None, 0, 3, 1, None, None) == 0
    assert lib.umnn_flow_sample_ll(None, None, 0, 3, None, None) == 0
    for args in ((None, p, 4, 3, 1, p, None), (p, None, 4, 3, 0, p, None), (p, p, 4, 3, 0, None, None), (p, p, 4, 0, 0, p, None),
                 (p, p, -1, 3, 0, p, None), (p, p, 4, 3, 2, p, None)):
        assert lib.umnn_flow_sample_lj_rows(*args) == _lib.EINVAL and b"flow sample lj" in lib.umnn_last_error()
    for args in ((None, p, 4, 3, p, None), (p, None, 4, 3, p, None), (p, p, 4, 3, None, None), (p, p, 4, 0, p, None), (p, p, -1, 3, p, None)):
        assert lib.umnn_flow_sample_ll(*args) == _lib.EINVAL and b"flow sample ll" in lib.umnn_last_error()
    net = _lib.MlpDesc()
    widths = [5, 50, 50, 1]
    net.n_linear = 3
    for i, w in enumerate(widths):
        net.widths[i] = w
    for l in range(3):
        net.W[l], net.b[l] = 0x1000, 0x1000

    def solve_lj(B, x, lj, first):
        return lib.umnn_cc_solve_lj(ctypes.byref(net), p, p, 3, None, p, None, 1, p, p, 20, B, 3, 4, 0, -50., 50., 1e-6, 32, x, 3, None, None,
                                    lj, first, None)
    assert solve_lj(0, p, p, 1) == 0                                   # empty batch: nothing to launch
    assert solve_lj(0, p, None, 0) == 0                                # (lj_row is nullable: then it is umnn_cc_solve)
    assert solve_lj(4, p, p, 2) == _lib.EINVAL and b"lj_first" in lib.umnn_last_error()
    assert solve_lj(4, None, p, 1) == _lib.EINVAL and b"null pointer" in lib.umnn_last_error()
