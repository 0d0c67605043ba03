"""The progressive MADE conditioner on the GPU: ``umnn_made_step`` per step against a float64 truth, its prefix discipline (NaN
ahead of the walk), batch / row-tile invariance, whole blocks of ``invert(conditioner="progressive")`` against ``"full"`` and the
hipGraph replay of ``GraphedSampler``.

Shapes: (a)-(d) of tests/test_progressive_cpu.py and (e) MADE(63, [128, 128], 252) at B = 37: a partial row tile and several K chunks
per wave.

Bounds.  Kernel against truth: 4 x the error of torch's own fp32 ``F.linear`` chain on the same device against the same float64
truth, both scaled by max |truth| (the margin is for another summation order).  Whole blocks: the round-trip bound of the existing
inverse tests -- sum over the blocks of TOL / min exp(s) f in float64 (``_flow_bound`` of tests/test_gpu_graph_sampling.py) -- for each
path against x, twice that between the two paths."""
import copy
import warnings

import numpy as np
import pytest
import torch

import umnn_amd
from tests.test_gpu_graph_sampling import TOL, _flow_bound
from umnn_amd import _lib
from umnn_amd.made import MADE, ConditionnalMADE, MaskedLinear

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
B0 = 37


def _build(name):
    torch.manual_seed(5)
    return {"a": lambda: MADE(5, [16, 16], 15), "b": lambda: MADE(17, [8, 8], 51),
            "c": lambda: MADE(6, [32, 24, 40], 12, natural_ordering=True, random=True),
            "d": lambda: ConditionnalMADE(4, 3, [20, 20], 14), "e": lambda: MADE(63, [128, 128], 252)}[name]()


_CASES = {}


def _case(name, gain):
    """(made on the device, x, context, float64 truth [B, E, d], error of torch's fp32 chain) -- computed once, never modified."""
    key = (name, gain)
    if key not in _CASES:
        made = _build(name)
        if gain != 1.:
            with torch.no_grad():
                for l in made.net:
                    if isinstance(l, MaskedLinear):
                        l.weight.mul_(gain)
        c = getattr(made, "cond_in", 0)
        d = made.nin - c
        g = torch.Generator().manual_seed(d)
        x = torch.randn(64, d, generator=g)
        ctx = torch.randn(64, c, generator=g) if c else None
        m64 = copy.deepcopy(made).double()
        umnn_amd.invalidate_caches(m64)
        with torch.no_grad():
            truth = (m64.raw(x.double(), ctx.double()) if c else m64.raw(x.double())).view(64, -1, d)
        made = made.to(DEV)
        with torch.no_grad():
            a = x.to(DEV) if ctx is None else torch.cat((ctx, x), 1).to(DEV)
            chain = made.net(a).view(64, -1, made.nin)[:, :, c:]          # torch's own fp32 F.linear chain on the masked weights
        scale = float(truth.abs().max())
        torch_err = float((chain.cpu().double() - truth).abs().max()) / scale
        _CASES[key] = (made, x.to(DEV), None if ctx is None else ctx.to(DEV), truth, scale, torch_err)
    return _CASES[key]


def _walk(made, x, ctx, ahead=float("nan"), row_tiles=0):
    """The kernel walk over the final ``x`` fed in progressively; columns >= j hold ``ahead`` before step j -> h[:, :, j] per step."""
    plan = made.progressive_plan(DEV)
    assert plan is not None and plan.desc is not None
    B, d = x.shape
    x_walk = torch.full_like(x, ahead)
    walk = plan.walk(x_walk, ctx, True)
    assert walk.kernel
    walk.row_tiles = row_tiles
    cols = []
    before = _lib.lib().umnn_made_launch_count()
    for j in range(d):
        cols.append(walk.step(j).view(B, -1, d)[:, :, j].clone())
        x_walk[:, j] = x[:, j]
    assert _lib.lib().umnn_made_launch_count() - before == d
    assert _lib.lib().umnn_last_made_kernel_name().decode().startswith("made_step<RT=")
    return torch.stack(cols, 2)                                              # [B, E, d]


# ---- 6. the kernel against the truth, per step -----------------------------------------------------------------------------------
@pytest.mark.parametrize("gain", [1., 3.])
@pytest.mark.parametrize("name", ["a", "b", "c", "d", "e"])
def test_kernel_against_the_truth_per_step(name, gain):
    """h[:, :, j] after step j against the float64 full pass on the final x, worst step; bound 4 x torch's fp32 chain error.
    Measured on an MI355X, kernel error / torch fp32 chain error (both scaled by max |truth|), weights x 1 and x 3:
    (a) 5.8e-8 / 6.6e-8 = 0.87, 1.5e-7 / 9.3e-8 = 1.60; (b) 0.53, 0.94; (c) 0.95, 0.67; (d) 0.85, 1.05; (e) 1.3e-7 / 2.0e-7 = 0.65, 0.70."""
    made, x, ctx, truth, scale, torch_err = _case(name, gain)
    h = _walk(made, x[:B0], None if ctx is None else ctx[:B0])
    per_step = (h.cpu().double() - truth[:B0]).abs().amax((0, 1)) / scale
    err = float(per_step.max())
    print(f"case {name} x{gain:g}: kernel {err:.2e} (worst step {int(per_step.argmax())}), torch fp32 chain {torch_err:.2e}, "
          f"ratio {err / torch_err if torch_err else float('inf'):.2f}")
    assert torch.isfinite(h).all()
    assert err <= 4 * torch_err


# ---- 7. never reads ahead --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["a", "b", "c", "d", "e"])
def test_never_reads_ahead(name):
    made, x, ctx, *_ = _case(name, 1.)
    ctx = None if ctx is None else ctx[:B0]
    h_nan = _walk(made, x[:B0], ctx, ahead=float("nan"))
    h_zero = _walk(made, x[:B0], ctx, ahead=0.)
    assert torch.isfinite(h_nan).all()
    assert torch.equal(h_nan, h_zero)


# ---- 8. batch and row-tile invariance --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["c", "d", "e"])
def test_batch_and_row_tile_invariance(name):
    made, x, ctx, *_ = _case(name, 1.)
    cut = lambda lo, hi: None if ctx is None else ctx[lo:hi].contiguous()
    h37 = _walk(made, x[:B0].contiguous(), cut(0, B0))
    h64 = _walk(made, x, ctx)
    assert torch.equal(h37, h64[:B0])
    for r in (0, 15, 16, B0 - 1):
        assert torch.equal(_walk(made, x[r:r + 1].contiguous(), cut(r, r + 1)), h37[r:r + 1]), r
    for rt in (1, 2, 4):
        assert torch.equal(_walk(made, x[:B0].contiguous(), cut(0, B0), row_tiles=rt), h37), rt


# ---- 9. whole blocks, progressive against full -----------------------------------------------------------------------------------
FLOWS = {"power": dict(d=6, hd=[50] * 4, he=[512, 512], E=30, n=50, nb_flow=1, B=50, cond_in=0),
         "d63": dict(d=63, hd=[50] * 4, he=[128, 128], E=4, n=30, nb_flow=1, B=64, cond_in=0),
         "cond": dict(d=3, hd=[50] * 4, he=[64, 64], E=30, n=20, nb_flow=2, B=33, cond_in=3)}


def _flow(name):
    f = FLOWS[name]
    torch.manual_seed(len(name))
    m = umnn_amd.UMNNMAFFlow(nb_flow=f["nb_flow"], nb_in=f["d"], hidden_derivative=f["hd"], hidden_embedding=f["he"], embedding_s=f["E"],
                             nb_steps=f["n"], solver="CCParallel", cond_in=f["cond_in"]).to(DEV).eval()
    for p in m.parameters():
        p.requires_grad_(False)
    g = torch.Generator().manual_seed(f["B"])
    x = (1.5 * torch.randn(f["B"], f["d"], generator=g)).to(DEV)
    ctx = torch.randn(f["B"], f["cond_in"], generator=g).to(DEV) if f["cond_in"] else None
    return f, m, x, ctx


@pytest.mark.parametrize("method", ["newton", "bracket"])
@pytest.mark.parametrize("name", sorted(FLOWS))
def test_whole_blocks_progressive_against_full(name, method):
    f, m, x, ctx = _flow(name)
    bound = _flow_bound(m, x, ctx)
    opts = dict(method="newton") if method == "newton" else dict(iter=10)
    lib = _lib.lib()
    with torch.no_grad(), warnings.catch_warnings(record=True) as said:
        warnings.simplefilter("always")
        z = m(x, context=ctx)
        x_full = m.invert(z, context=ctx, conditioner="full", **opts)
        made0, solve0 = lib.umnn_made_launch_count(), lib.umnn_launch_count()
        x_prog = m.invert(z, context=ctx, conditioner="progressive", **opts)
        made1, solve1 = lib.umnn_made_launch_count(), lib.umnn_launch_count()
    assert umnn_amd.path_taken() == "hip"
    assert not [w for w in said if "progressive" in str(w.message)], "no fallback is announced: the kernel takes these"
    assert made1 - made0 == f["nb_flow"] * f["d"], "one conditioner step launch per dimension and block"
    assert solve1 - solve0 == f["nb_flow"] * f["d"], "and one solve launch: two launches per dimension"
    assert lib.umnn_last_made_kernel_name().decode().startswith("made_step<RT=")
    e_full, e_prog, diff = (float((a - b).abs().max()) for a, b in ((x_full, x), (x_prog, x), (x_full, x_prog)))
    print(f"{name} {method}: |full - x| {e_full:.2e}, |progressive - x| {e_prog:.2e}, |full - progressive| {diff:.2e}, bound {bound:.2e}")
    assert x_prog.shape == x.shape and x_prog.dtype == torch.float32
    assert e_full <= bound and e_prog <= bound
    assert diff <= 2 * bound


# ---- 10. graph replay ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["power", "cond"])
def test_graphed_sampler_replays_the_progressive_walk(name):
    f, m, x, ctx = _flow(name)
    n = 64
    g = torch.Generator().manual_seed(1)
    z = torch.randn(n, f["d"], generator=g).to(DEV)
    c = torch.randn(n, f["cond_in"], generator=g).to(DEV) if f["cond_in"] else None
    lib = _lib.lib()
    with torch.no_grad():
        eager = m.invert(z, context=c, method="newton", conditioner="progressive")
        sampler = umnn_amd.GraphedSampler(m, n, context=c, method="newton", conditioner="progressive")
        assert sampler.captures == 1 and umnn_amd.path_taken() == "hip"
        made0, solve0 = lib.umnn_made_launch_count(), lib.umnn_launch_count()
        x1 = sampler(z=z, context=c).clone()
        x2 = sampler(z=z, context=c)
        assert (lib.umnn_made_launch_count(), lib.umnn_launch_count()) == (made0, solve0), "a replay makes no launch from the host"
        assert torch.equal(x1, eager) and torch.equal(x2, eager)
        # an optimizer-style in-place update: the versions move, the sampler re-captures and the replay sees the new weights
        for blk in m.nets:
            for p in blk.net.made.parameters():
                p.mul_(1.25)
        x3 = sampler(z=z, context=c).clone()
        assert sampler.captures == 2
        eager_new = m.invert(z, context=c, method="newton", conditioner="progressive")
        assert torch.equal(x3, eager_new) and not torch.equal(x3, eager)
        sampler(z=z, context=c)
        assert sampler.captures == 2
        with pytest.raises(ValueError):
            umnn_amd.GraphedSampler(m, n, context=c, method="jacobi", sweep_tol=0, max_sweeps=2, conditioner="progressive")
