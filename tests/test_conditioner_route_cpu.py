"""The conditioner's one route decision against the hand-written table of tests/_made_route_cases.py, and its one cache rule on host
tensors (no GPU: ``conditioner_route`` is a function of values, and the caches key on tensor versions and pointers)."""
import numpy as np
import pytest
import torch

from tests import _made_route_cases as C
from umnn_amd import made as M


@pytest.mark.parametrize("case", C.CASES, ids=[c["id"] for c in C.CASES])
def test_route_table(case):
    opts = M.MadeOptions(**{**C.DEFAULTS, **case["opts"]})
    route = M.conditioner_route(case["rows"], case["widths"], case["n_out"], opts=opts, **case["flags"])
    assert tuple(route) == case["expect"]
    assert (route.name, route.no_cat, route.lib_out) == case["expect"]


def test_table_holds_every_arm_and_its_ids_are_unique():
    assert len({c["id"] for c in C.CASES}) == len(C.CASES)
    assert {c["expect"][0] for c in C.CASES} == set(C.LAUNCHES)
    assert {c["expect"] for c in C.CASES} >= {("layered", True, False), ("layered", False, True), ("layered", True, True)}


def test_defaults_are_what_an_empty_environment_gives():
    have = M._options_from_env({})
    assert {k: getattr(have, k) for k in C.DEFAULTS if k != "addmm_act"} == {k: v for k, v in C.DEFAULTS.items() if k != "addmm_act"}
    assert have.addmm_act == hasattr(torch, "_addmm_activation") and have.probe is None


def test_modules_have_the_widths_the_table_writes():
    """The nets the GPU test builds for a case have that case's (in_features, out_features) and surviving width."""
    for case in C.CASES:
        if case["gpu"] is None:
            continue
        net = build(case["gpu"]["net"])
        assert [(l.in_features, l.out_features) for l in net._masked_layers()] == case["widths"], case["id"]
        n_out = net.nin_non_cond * (net.nout // net.nin) if isinstance(net, M.ConditionnalMADE) else net.nout
        assert n_out == case["n_out"], case["id"]


def build(spec):
    if spec[0] == "COND":
        return M.ConditionnalMADE(spec[1], spec[2], spec[3], spec[4], num_masks=1, natural_ordering=True)
    return M.MADE(spec[1], spec[2], spec[3], num_masks=1, natural_ordering=True)


def test_setters_change_the_one_record_and_nothing_else():
    old = M.dataclasses.replace(M._OPTIONS)
    try:
        M.set_made_fast_path(False)
        assert M.get_made_fast_path() is False and M._OPTIONS.fast is False
        M.set_made_fused(False, max_rows=7, wide_out=True, hybrid=True, layered=False)
        assert (M._OPTIONS.fused, M._OPTIONS.max_rows, M._OPTIONS.wide_out, M._OPTIONS.hybrid, M._OPTIONS.layered) == (False, 7, True, True, False)
        M.set_made_fused(True)          # (None leaves a switch as it is)
        assert (M._OPTIONS.fused, M._OPTIONS.max_rows, M._OPTIONS.wide_out, M._OPTIONS.hybrid, M._OPTIONS.layered) == (True, 7, True, True, False)
        M._TRAIN_FUSED["enabled"] = False       # (the earlier spelling of the one-node chain's switch: the same field)
        assert M._OPTIONS.train_fused is False and M._TRAIN_FUSED["enabled"] is False
    finally:
        M.set_made_fast_path(old.fast)
        M.set_made_fused(old.fused, old.max_rows, old.wide_out, old.hybrid, old.layered)
        M._TRAIN_FUSED["enabled"] = old.train_fused
    assert M._OPTIONS == old


def test_host_input_takes_the_plain_chain_without_a_library_load():
    """A CPU call must decide without the probe (the library load would raise on a box without the HIP library)."""
    torch.manual_seed(0)
    net = build(("COND", 4, 3, [9], 14))
    x, ctx = torch.randn(6, 4), torch.randn(6, 3)
    probe = M._OPTIONS.probe
    with torch.no_grad():
        out = net.raw(x, ctx)
        full = net.net(torch.cat((ctx, x), 1)).view(6, 2, 7)[:, :, 3:].reshape(6, -1)
        out16 = net.raw(x, ctx, out_dtype=torch.bfloat16)
    assert M._OPTIONS.probe is probe
    assert out.shape == (6, 8) and float((out - full).abs().max()) <= 1e-6 * float(full.abs().max())
    assert out16.dtype == torch.bfloat16 and torch.equal(out16, out.bfloat16())
    assert torch.equal(net.forward(x, ctx), net.raw(x, ctx)) and M.MADE.raw_rows(net, x, torch.tensor([0, 1])) is None


# ---------------------------------------------------------------------------------------------------------------- the cache rule
def _layer():
    torch.manual_seed(1)
    l = M.MaskedLinear(6, 10)
    l.set_mask(np.tril(np.ones((6, 10), dtype=bool)))
    return l


GETTERS = {"masked_weight": lambda l, rows=None: l.masked_weight(), "packed_bf16": lambda l, rows=None: l.packed_bf16(rows),
           "packed_fragments": lambda l, rows=None: l.packed_fragments(rows)}


@pytest.mark.parametrize("name", list(GETTERS))
def test_cache_hit_and_every_invalidation(name):
    get, l = GETTERS[name], _layer()
    with torch.no_grad():
        first = get(l)
        assert get(l) is first, "a hit on an equal key returns the stored object"
        l.weight.mul_(1.5)                                  # in place: the version moves
        second = get(l)
        assert second is not first and get(l) is second
        l.bias.add_(1.0)
        third = get(l)
        if name == "masked_weight":                         # (holds no bias: its key does not name it)
            assert third is second
        else:
            assert third is not second and get(l) is third
        l.set_mask(np.triu(np.ones((6, 10), dtype=bool)))
        fourth = get(l)
        assert fourth is not third and get(l) is fourth
        l.invalidate_caches()
        fifth = get(l)
        assert fifth is not fourth and get(l) is fifth
        flat = lambda v: torch.cat([t.float().reshape(-1) for t in (v if isinstance(v, tuple) else (v,))])
        assert torch.equal(flat(fifth), flat(fourth)) and not torch.equal(flat(fourth), flat(third)), "same inputs, same value; new mask, new value"


@pytest.mark.parametrize("name", ["packed_bf16", "packed_fragments"])
def test_cache_rows_are_part_of_the_key(name):
    get, l = GETTERS[name], _layer()
    rows, other = torch.tensor([1, 4, 7]), torch.tensor([1, 4, 7])
    with torch.no_grad():
        full = get(l)
        sel = get(l, rows)
        assert sel is not full and get(l, rows) is sel
        assert get(l, other) is not sel, "another rows tensor is another key (the pointer, not the content)"
        width = (lambda v: v[1].shape[0]) if name == "packed_fragments" else (lambda v: v.shape[0])
        assert width(sel) == 3 and width(full) == 10


def test_row_selection_from_the_full_packed_weight_leaves_the_full_entry():
    """What ``raw_rows`` does per flow dimension: select from the cached FULL operand; the layer's cache keeps the full entry."""
    l = _layer()
    with torch.no_grad():
        full = l.packed_bf16(None)
        for j in range(3):
            rows = torch.tensor([j, j + 3])
            sel = l.packed_bf16(None).index_select(0, rows)
            assert torch.equal(sel, full[rows]) and l.packed_bf16(None) is full


def test_masked_weight_under_autograd_is_the_live_product():
    l = _layer()
    w = l.masked_weight()
    assert w.grad_fn is not None and l.masked_weight() is not w
    with torch.no_grad():
        cached = l.masked_weight()
    assert cached.grad_fn is None and torch.equal(cached, w.detach())
    l.weight.requires_grad_(False)
    assert l.masked_weight() is cached, "frozen weights: the cached product in grad mode too"


def test_progressive_plan_follows_the_same_rule():
    torch.manual_seed(2)
    net = build(("MADE", 4, [9, 9], 8))
    dev = torch.device("cpu")
    with torch.no_grad():
        plan = net.progressive_plan(dev)
        assert plan is not None and net.progressive_plan(dev) is plan
        net.net[2].bias.add_(1.0)
        again = net.progressive_plan(dev)
        assert again is not plan and net.progressive_plan(dev) is again
        M.invalidate_caches(net)
        assert net.progressive_plan(dev) is not again
