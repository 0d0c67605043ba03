"""The progressive MADE conditioner of the sequential sampling walk, without a GPU: the plan against brute force from the mask
buffers, the plain-torch walk against the full pass in float64, ``invert(conditioner="progressive")`` against ``"full"`` on host
tensors, the option handling and ``umnn_made_step``'s argument validation.

Shapes: the smallest at which the walk can go wrong -- (a) unused top-degree units, (b) H < d: steps with no new unit, (c) scattered
random degrees over three layers, (d) a conditional MADE, whose step 0 takes several degrees at once.

Bounds.  The float64 walk sums at most 40 terms per unit in another order than the full pass: 1e-12 (3e-17 measured).  A whole
flow: each path is held to the round-trip bound of tests/test_inverse_cpu.py -- sum over the blocks of TOL / min exp(s) f from the
float64 oracle of tests/_inverse_truth.py -- and the two paths to twice that of one another."""
import copy
import ctypes
import warnings

import numpy as np
import pytest
import torch

import umnn_amd
from tests import _inverse_truth as T
from tests.test_inverse_cpu import TOL
from umnn_amd import _lib, integral
from umnn_amd.made import MADE, ConditionnalMADE, MaskedLinear

CPU = torch.device("cpu")


def _cases():
    torch.manual_seed(5)
    return {"a": MADE(5, [16, 16], 15), "b": MADE(17, [8, 8], 51),
            "c": MADE(6, [32, 24, 40], 12, natural_ordering=True, random=True), "d": ConditionnalMADE(4, 3, [20, 20], 14)}


CASES = _cases()


def _layers(made):
    return [l for l in made.net if isinstance(l, MaskedLinear)]


# ---- 1. the plan against brute force from the mask buffers ---------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(CASES))
def test_plan_partitions_the_needed_units_and_its_prefixes_cover_every_weight(name):
    made = CASES[name]
    plan = made.progressive_plan(CPU)
    assert plan is not None
    layers = _layers(made)
    L, nin = len(made.hidden_sizes), made.nin
    c = getattr(made, "cond_in", 0)
    d, E = nin - c, made.nout // nin
    assert (plan.c, plan.d, plan.E) == (c, d, E) and plan.steps.shape == (d, L + 1, 3) and plan.steps.dtype == np.int32
    masked = [(l.mask * l.weight).detach() for l in layers]
    for l in range(L):
        order = plan.orders[l].numpy()
        deg = np.asarray(made.m[l])
        assert sorted(order.tolist()) == list(range(len(deg))) and np.all(np.diff(deg[order]) >= 0)
        assert np.all(np.diff(order)[np.diff(deg[order]) == 0] > 0), "the sort is stable"
        # the new-unit ranges are consecutive from 0 and end exactly at the units of degree <= nin - 2
        seen = 0
        for j in range(d):
            lo, hi, _ = plan.steps[j, l]
            assert lo == seen and hi >= lo
            assert np.all(deg[order[lo:hi]] <= c + j - 1) and (hi == len(deg) or deg[order[hi]] > c + j - 1)
            seen = hi
        assert seen == int((deg <= nin - 2).sum())
        # the permuted weights are the masked weights, zero padded
        W = masked[l][plan.orders[l]]
        W = W if l == 0 else W[:, plan.orders[l - 1]]
        assert torch.equal(plan.W[l][:, :W.shape[1]], W) and not plan.W[l][:, W.shape[1]:].any()
        assert torch.equal(plan.b[l], layers[l].bias.detach()[plan.orders[l]])
        assert plan.ldk[l] % 4 == 0 and plan.ldk[l] >= W.shape[1]
        # every prefix covers every non-zero masked weight of the units it serves, and nothing not yet computed
        for j in range(d):
            lo, hi, pre = plan.steps[j, l]
            assert not plan.W[l][lo:hi, pre:].any()
            assert pre == c + j if l == 0 else pre <= plan.steps[j, l - 1, 1]
    for j in range(d):
        lo, hi, pre = plan.steps[j, L]
        rows = torch.tensor([e * nin + c + j for e in range(E)])
        Wj = masked[L][rows][:, plan.orders[L - 1]]
        assert (lo, hi) == (0, E) and pre <= plan.steps[j, L - 1, 1]
        assert torch.equal(plan.W[L][j][:, :Wj.shape[1]], Wj) and not plan.W[L][j][:, pre:].any()
        assert torch.equal(plan.b[L][j], layers[L].bias.detach()[rows])
    assert plan.max_new == int((plan.steps[:, :L, 1] - plan.steps[:, :L, 0]).max())
    assert plan.desc is None, "host weights: no kernel descriptor"


def test_plan_cache_and_eligibility():
    made = copy.deepcopy(CASES["a"])
    p1 = made.progressive_plan(CPU)
    assert made.progressive_plan(CPU) is p1
    with torch.no_grad():
        _layers(made)[1].weight.mul_(2.)                    # a versioned write: the key moves
    p2 = made.progressive_plan(CPU)
    assert p2 is not p1 and torch.equal(p2.W[1], 2. * p1.W[1])
    _layers(made)[0].weight.data.mul_(2.)                   # invisible to the key ...
    assert made.progressive_plan(CPU) is p2
    umnn_amd.invalidate_caches(made)                        # ... until the caches are dropped
    p3 = made.progressive_plan(CPU)
    assert p3 is not p2 and torch.equal(p3.W[0], 2. * p2.W[0])
    _layers(made)[0].set_mask(np.zeros((5, 16), dtype=bool))
    assert not made.progressive_plan(CPU).W[0].any()
    assert copy.deepcopy(made).progressive_plan(CPU) is not None
    torch.manual_seed(1)
    assert MADE(6, [16, 16], 12, random=True).progressive_plan(CPU) is None, "random input order"
    assert MADE(6, [16, 16], 12, num_masks=2, natural_ordering=True, random=True).progressive_plan(CPU) is None, "several masks"
    assert MADE(5, [16, 16], 15).bfloat16().progressive_plan(CPU) is None, "bf16 weights"


# ---- 2. the walk against the full pass in float64 -------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(CASES))
def test_walk_equals_the_full_pass_in_float64(name):
    made = copy.deepcopy(CASES[name]).double()
    umnn_amd.invalidate_caches(made)
    plan = made.progressive_plan(CPU)
    B, d = 9, plan.d
    g = torch.Generator().manual_seed(d)
    x = torch.randn(B, d, generator=g, dtype=torch.float64)
    ctx = torch.randn(B, plan.c, generator=g, dtype=torch.float64) if plan.c else None
    with torch.no_grad():
        truth = (made.raw(x, ctx) if plan.c else made.raw(x)).view(B, -1, d)
        x_walk = torch.full_like(x, float("nan"))           # the final x is fed in progressively: nothing is read ahead
        walk = plan.walk(x_walk, ctx, False)
        worst = 0.
        for j in range(d):
            h = walk.step(j).view(B, -1, d)
            worst = max(worst, float((h[:, :, j] - truth[:, :, j]).abs().max()))
            x_walk[:, j] = x[:, j]
    print(f"case {name}: max |walk - full pass| {worst:.1e}")
    assert worst <= 1e-12


# ---- 3. progressive against full on a whole flow --------------------------------------------------------------------------------
def _bound64(m, x, ctx):
    """sum over the blocks of TOL / min exp(s) f from the model's own float64 copy (a conditional flow: the oracle blocks of
    tests/_inverse_truth.py are unconditional)."""
    m64 = copy.deepcopy(m).double()
    umnn_amd.invalidate_caches(m64)
    xi, total = x.double(), 0.
    with torch.no_grad():
        for blk in m64.nets:
            z, lj = blk._transform(xi, None if ctx is None else ctx.double(), want_jac=True)
            total += TOL / float(torch.exp(lj.min()))
            xi = torch.flip(z, [1])
    return total


@pytest.mark.parametrize("cond_in", [0, 3])
def test_progressive_flow_inversion_against_full(cond_in):
    torch.manual_seed(11 + cond_in)
    m = umnn_amd.UMNNMAFFlow(nb_flow=2, nb_in=5, hidden_derivative=[40] * 3, hidden_embedding=[32, 32], embedding_s=8, nb_steps=30,
                             solver="CCParallel", cond_in=cond_in).eval()
    g = torch.Generator().manual_seed(3)
    x = 1.5 * torch.randn(24, 5, generator=g)
    ctx = torch.randn(24, cond_in, generator=g) if cond_in else None
    if cond_in:
        bound = _bound64(m, x, ctx)
    else:
        blocks = T.blocks_from_state_dict(m.state_dict(), 2)
        bound = sum(TOL / v for v in T.flow_min_sf(blocks, x.numpy(), 30))
    assert 1e-5 < bound < 1e-2, bound
    with torch.no_grad(), warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        z = m(x, context=ctx)
        x_full = m.invert(z, context=ctx, method="newton", conditioner="full")
        x_prog = m.invert(z, context=ctx, method="newton", conditioner="progressive")
        assert torch.equal(x_full, m.invert(z, context=ctx, method="newton")), "'full' is the default"
        b_full = m.invert(z, context=ctx, iter=6)
        b_prog = m.invert(z, context=ctx, iter=6, conditioner="progressive")
    e_full, e_prog, diff = (float((a - b).abs().max()) for a, b in ((x_full, x), (x_prog, x), (x_full, x_prog)))
    print(f"cond_in={cond_in}: |full - x| {e_full:.2e}, |progressive - x| {e_prog:.2e}, |full - progressive| {diff:.2e}, bound {bound:.2e}")
    assert e_full <= bound and e_prog <= bound and diff <= 2 * bound
    # the bracket search lands on a grid of 100 / 9^iter: the conditioner's rounding may move a row by one cell at the most
    assert float((b_full - b_prog).abs().max()) <= 2 * 100. / 9 ** 6 + 2 * bound
    x1 = m.nets[0].invert(m.nets[0](x, context=ctx), context=ctx, method="newton", conditioner="progressive")
    assert float((x1 - x).abs().max()) <= bound


# ---- 4. option handling -----------------------------------------------------------------------------------------------------------
def test_option_handling():
    torch.manual_seed(2)
    m = umnn_amd.UMNNMAFFlow(nb_flow=1, nb_in=3, hidden_derivative=[20, 20], hidden_embedding=[16, 16], embedding_s=4, nb_steps=20,
                             solver="CCParallel").eval()
    z = torch.randn(4, 3)
    for target in (m, m.nets[0]):
        with pytest.raises(ValueError, match="progressive"):
            target.invert(z, method="jacobi", conditioner="progressive")
        with pytest.raises(ValueError, match="conditioner"):
            target.invert(z, method="newton", conditioner="fast")
        with pytest.raises(ValueError, match="conditioner"):
            target.invert(z, conditioner=None)
    with torch.no_grad(), warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        assert torch.equal(m.invert(z, method="jacobi", conditioner="full"), m.invert(z, method="jacobi"))
        assert m.sample(5, conditioner="progressive").shape == (5, 3)


def test_a_random_input_order_falls_back_to_full_with_one_warning():
    torch.manual_seed(4)
    m = umnn_amd.UMNNMAFFlow(nb_flow=1, nb_in=4, hidden_derivative=[20, 20], hidden_embedding=[16, 16], embedding_s=4, nb_steps=20,
                             solver="CCParallel").eval()
    blk = m.nets[0]
    torch.manual_seed(8)
    blk.net.made = MADE(4, [16, 16], 16, random=True)       # natural_ordering=False: a random input order
    assert not np.array_equal(blk.net.made.m[-1], np.arange(4))
    z = torch.randn(6, 4)
    integral._warned.discard("progressive-ineligible")
    with torch.no_grad(), warnings.catch_warnings(record=True) as rec:
        warnings.simplefilter("always")
        x_prog = m.invert(z, method="newton", conditioner="progressive")
        x_again = m.invert(z, method="newton", conditioner="progressive")
        x_full = m.invert(z, method="newton", conditioner="full")
    said = [w for w in rec if "conditioner='progressive'" in str(w.message)]
    assert len(said) == 1 and issubclass(said[0].category, RuntimeWarning)
    assert torch.equal(x_prog, x_full) and torch.equal(x_again, x_full)


# ---- 5. umnn_made_step validates its arguments without a GPU ---------------------------------------------------------------------
def _desc(d=5, c=0, E=3, widths=(16, 16), steps=None):
    L = len(widths)
    p = _lib.MadePlan()
    p.n_hidden, p.d, p.c, p.E = L, d, c, E
    for l, w in enumerate(widths):
        p.width[l] = w
    for l, k in enumerate((c + d,) + tuple(widths)):
        p.ldk[l] = -(-k // 4) * 4
        p.W[l], p.b[l] = 0x1000, 0x1000
    if steps is None:
        steps = np.zeros((d, L + 1, 3), dtype=np.int32)
        steps[:, L, 1] = E
    p._keep = steps
    p.steps = steps.ctypes.data
    return p


def test_made_step_validates_without_a_gpu():
    lib = _lib.lib()
    ptr = ctypes.c_void_p(0x1000)
    act = (ctypes.c_void_p * 8)(*([0x1000] * 8))
    p = _desc()
    call = lambda plan, j, ctx, x, a, h, B, rt=0: lib.umnn_made_step(None if plan is None else ctypes.byref(plan), j, ctx, x, a, h, B, rt, None)
    assert call(None, 0, None, ptr, act, ptr, 4) == _lib.EINVAL
    for j in (-1, 5, 99):
        assert call(p, j, None, ptr, act, ptr, 4) == _lib.EINVAL and b"j outside" in lib.umnn_last_error()
    assert call(p, 0, None, None, act, ptr, 4) == _lib.EINVAL and b"non-null" in lib.umnn_last_error()
    assert call(p, 0, None, ptr, act, None, 4) == _lib.EINVAL
    assert call(p, 0, None, ptr, None, ptr, 4) == _lib.EINVAL
    assert call(p, 0, None, ptr, act, ptr, -1) == _lib.EINVAL
    assert call(p, 0, None, ptr, act, ptr, 4, 3) == _lib.EINVAL, "row_tiles 0 | 1 | 2 | 4"
    assert call(_desc(c=2), 0, None, ptr, act, ptr, 4) == _lib.EINVAL, "a conditional plan needs the context"
    # an empty batch is a no-op, not an error (and touches no device)
    assert call(p, 0, None, ptr, act, ptr, 0) == 0
    bad = _desc()
    bad.ldk[1] = 18
    assert call(bad, 0, None, ptr, act, ptr, 4) == _lib.EINVAL
    steps = np.zeros((5, 3, 3), dtype=np.int32)
    steps[:, 2, 1] = 3
    steps[2, 0] = (0, 17, 2)                                  # more units than the layer has
    assert call(_desc(steps=steps), 2, None, ptr, act, ptr, 4) == _lib.EINVAL and b"step table" in lib.umnn_last_error()
    steps[2, 0] = (0, 4, 3)                                   # a prefix past column j of x
    assert call(_desc(steps=steps), 2, None, ptr, act, ptr, 4) == _lib.EINVAL
    steps[2, 0] = (0, 4, 2)
    steps[2, 1] = (0, 4, 5)                                   # a prefix past the units computed so far
    assert call(_desc(steps=steps), 2, None, ptr, act, ptr, 4) == _lib.EINVAL
    # what the kernel does not hold is refused as unsupported: a new-unit slice wider than its LDS hand-off, nine hidden layers
    wide = np.zeros((5, 3, 3), dtype=np.int32)
    wide[:, 2, 1] = 3
    wide[1, 0] = (0, _lib.MADE_STEP_MAX_NEW + 1, 1)
    assert call(_desc(widths=(512, 16), steps=wide), 1, None, ptr, act, ptr, 4) == _lib.EUNSUPPORTED
    deep = _desc()
    deep.n_hidden = 9
    assert call(deep, 0, None, ptr, act, ptr, 4) == _lib.EUNSUPPORTED
