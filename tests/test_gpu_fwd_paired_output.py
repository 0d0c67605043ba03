"""The output stage of the two-tile forward waves runs once per wave: both tiles' output-layer sums go through ONE lane-group
reduction (tile 0 ends in lane groups 0 and 2, tile 1 in groups 1 and 3) and one output activation / 1/f / quadrature fma
(umnn_amd/csrc/cc_fwd_shared.h: group_allreduce_pair, group_unpair).  Same additions in the same order as the per-tile stage it
replaces, so every output keeps its bits.

Shape: 521 rows x d = 63 = 32 823 integrals = 2052 tiles -- just above the 2048 tiles at which a 256-CU part picks the pipelined
loop by itself; the last group is ragged (23 of 32 integrals: tile 1 of the last wave holds 7 live lanes) and, the group count
being odd against four groups per workgroup, whole waves of the last workgroup are dead.

Reference arithmetic: models/UMNN/ParallelNeuralIntegral.py:49-65 (quadrature), UMNNMAF.py:76-139 (z, log_jac),
UMNNMAFFlow.py:109-119 (ll) as restated by oracle/cc_oracle.py.
"""
import functools

import numpy as np
import pytest
import torch

from oracle import cc_oracle as O
from tests import _util as U
from tests.test_gpu_forward import TOL

pytestmark = pytest.mark.gpu

B, D, E = 521, 63, 30
HIDDEN = {"w50": [50] * 4, "w56": [56] * 4}          # LIVE = 13, merged 20-slot plan / LIVE = 0, 24-slot plan
CASES = [(w, relu, n, inv_f) for w in HIDDEN for relu in (False, True) for n in (6, 100) for inv_f in (False, True)]
CASE_IDS = [f"{w}-{'relu' if relu else 'leaky'}-n{n}-{'invf' if inv_f else 'f'}" for w, relu, n, inv_f in CASES]
MODES = ["f16x3", "bf16x3"]
FAMILY = {"f16x3": "cc_fwd_f16<", "bf16x3": "cc_fwd_bf16<"}


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


@pytest.fixture()
def restore_precision():
    import umnn_amd
    old = umnn_amd.get_forward_precision()
    yield
    umnn_amd.set_forward_precision(old)


def _t(a, dev):
    return torch.from_numpy(np.array(a)).to(dev)            # (a copy: the shared arrays are read-only)


def _kname():
    from umnn_amd import _lib
    return _lib.lib().umnn_last_kernel_name().decode()


@functools.lru_cache(maxsize=None)
def _problem(width, relu):
    """Weights and inputs of one integrand (host arrays; shared by every test of that integrand, never modified).

    Weights and biases are drawn as torch.nn.Linear draws them, uniform in +-1/sqrt(fan_in): what every integrand of this project
    starts from and what bench.py times.  (Not the Gaussian 1.6/sqrt(fan_in) weights of the 23-row tests of test_gpu_forward.py:
    their gain of ~1.3 per layer makes sum |w a| / |sum w a| large in the tails of 32 823 integrals, and the two-piece modes -- whose
    error is relative to sum |w a| -- and the fp32 oracle itself then sit AT the 1e-4 tolerance: measured with the kernels from
    before the paired output stage and with these, identical figures, up to 1.1e-4 on f(x) under bf16x3 and 3.7e-4 on the 1/f
    integral under f16x3.  That is the arithmetic modes' conditioning, which test_gpu_forward.py covers, not this file's subject.)"""
    rng = np.random.RandomState(1000 + 2 * HIDDEN[width][0] + relu)
    sizes = [1 + E] + HIDDEN[width] + [1]
    Ws = [rng.uniform(-1, 1, (sizes[i + 1], sizes[i])).astype(np.float32) / np.float32(np.sqrt(sizes[i])) for i in range(len(sizes) - 1)]
    bs = [rng.uniform(-1, 1, sizes[i + 1]).astype(np.float32) / np.float32(np.sqrt(sizes[i])) for i in range(len(sizes) - 1)]
    x = (rng.randn(B, D) * 2).astype(np.float32)
    h = rng.randn(B, E * D).astype(np.float32)
    sc = np.linspace(-0.3, 0.4, D).astype(np.float32)
    for a in Ws + bs + [x, h, sc]:
        a.setflags(write=False)
    return Ws, bs, x, h, sc


def _spec(width, relu, dev):
    from umnn_amd import _lib
    from umnn_amd.nets import MlpSpec
    Ws, bs = _problem(width, relu)[:2]
    lin = []
    for W, b in zip(Ws, bs):
        m = torch.nn.Linear(W.shape[1], W.shape[0])
        with torch.no_grad():
            m.weight.copy_(torch.from_numpy(W.copy()))
            m.bias.copy_(torch.from_numpy(b.copy()))
        lin.append(m.to(dev))
    return MlpSpec(lin, _lib.ACT_RELU if relu else _lib.ACT_LEAKY_RELU, _lib.OUT_ELU_PLUS_ONE)


@functools.lru_cache(maxsize=None)
def _oracle(width, relu, n, inv_f):
    """F, f(x), f(0) and -- plain integrand only, the flow entry points have no 1/f -- z, log_jac, ll.  Once per case, in row chunks
    (the oracle evaluates all n + 1 nodes of its rows as one batch)."""
    Ws, bs, x, h, sc = _problem(width, relu)
    net = O.Net(Ws, bs, O.RELU if relu else O.LEAKY, O.ELU1)
    x0 = np.zeros_like(x)
    F = np.concatenate([O.integrate_parallel(net, x0[i:i + 64], x[i:i + 64], h[i:i + 64], n, inv_f=inv_f) for i in range(0, B, 64)])
    ref = {"F": F, "fx": O.integrand(net, x, h), "fx0": O.integrand(net, x0, h)}
    if not inv_f:
        ref["z"] = np.exp(sc)[None, :] * (F + h.reshape(B, -1, D)[:, 0, :])
        ref["lj"] = np.log(ref["fx"] + np.float32(1e-10)) + sc[None, :]
        ref["ll"] = ref["lj"].sum(1) + np.float32(-.5) * (np.log(np.float32(np.pi) * np.float32(2)) + ref["z"] ** 2).sum(1)
    return ref


def _run(spec, x, h, sc, n, inv_f, flow=True):
    """Every output the forward kernel writes: F, f(x), f(x0) from the quadrature entry point; z, log_jac from the flow-block entry
    point and ll (with its z) from the one-pass log-likelihood (plain integrand only).  -> (dict of host arrays, kernel names)."""
    from umnn_amd import integral as I
    out, names = {}, []
    F, fx, fx0 = I.hip_forward(spec, None, x, h, n, inv_f=inv_f)
    names.append(_kname())
    out.update(F=F, fx=fx, fx0=fx0)
    if flow and not inv_f:
        z, lj = I.hip_flow_block(spec, x, h, sc, n)[:2]
        names.append(_kname())
        ll = torch.empty(x.shape[0], device=x.device, dtype=torch.float32)
        scratch = torch.empty_like(x)
        z1 = I.hip_flow_ll_block(spec, x, h, sc, n, False, True, True, ll, scratch)
        names.append(_kname())
        out.update(z=z, lj=lj, ll=ll, z_ll=z1)
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in out.items()}, names


@functools.lru_cache(maxsize=None)
def _gpu(width, relu, n, inv_f, mode, pipe):
    """One (case, arithmetic mode, loop) on the GPU with two tiles per wave; cached, so the tests below share the launches."""
    import umnn_amd
    from umnn_amd import _lib
    dev = torch.device("cuda:0")
    _, _, x, h, sc = _problem(width, relu)
    old = umnn_amd.get_forward_precision()
    saved = {k: _lib.get_option(k) for k in ("fwd_pipe", "fwd_p", "fwd_ns")}
    try:
        umnn_amd.set_forward_precision(mode)
        _lib.set_option("fwd_pipe", pipe)
        _lib.set_option("fwd_p", 2)
        _lib.set_option("fwd_ns", 1)
        return _run(_spec(width, relu, dev), _t(x, dev), _t(h, dev), _t(sc, dev), n, inv_f)
    finally:
        umnn_amd.set_forward_precision(old)
        for k, v in saved.items():
            _lib.set_option(k, v)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("width,relu,n,inv_f", CASES, ids=CASE_IDS)
def test_pipelined_and_plain_two_tile_loops_agree_bit_for_bit(width, relu, n, inv_f, mode, dev):
    """fwd_pipe = 1 against fwd_pipe = 0, both with two tiles per wave: F, f(x), f(x0), z, log_jac and the one-pass ll."""
    piped, names1 = _gpu(width, relu, n, inv_f, mode, 1)
    plain, names0 = _gpu(width, relu, n, inv_f, mode, 0)
    assert all(nm.startswith(FAMILY[mode]) and "PIPE" in nm and "P=2" in nm for nm in names1), names1
    assert all(nm.startswith(FAMILY[mode]) and "PIPE" not in nm and "P=2" in nm for nm in names0), names0
    assert set(piped) == set(plain) and len(piped) == (3 if inv_f else 7)
    for k in piped:
        assert np.array_equal(piped[k], plain[k], equal_nan=True), k
    if not inv_f:
        assert np.array_equal(piped["z"], piped["z_ll"])


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("width,relu,n,inv_f", CASES, ids=CASE_IDS)
def test_two_tile_outputs_against_oracle(width, relu, n, inv_f, mode, dev):
    """Both loops against the oracle, at the tolerance of tests/test_gpu_forward.py."""
    ref = _oracle(width, relu, n, inv_f)
    for pipe in (1, 0):
        got = _gpu(width, relu, n, inv_f, mode, pipe)[0]
        for k in ("F", "fx", "fx0") + (() if inv_f else ("z", "ll")):
            err = U.rel_err(got[k], ref[k])
            print(f"{mode} pipe={pipe} {k}: rel err {err:.3e}")
            assert err < TOL, (k, pipe, err)
        if not inv_f:
            assert np.all(np.abs(got["lj"] - ref["lj"]) <= TOL * np.maximum(1.0, np.abs(ref["lj"])))


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("width", list(HIDDEN))
def test_planner_picks_the_pipelined_loop_at_this_size(width, mode, dev, restore_precision):
    """No launch option set: 2052 tiles select the pipelined two-tile loop (on a part of at most 256 CUs), with the bits of the
    forced plan."""
    import umnn_amd
    if torch.cuda.get_device_properties(dev).multi_processor_count > 256:
        pytest.skip("more than 256 CUs: 2052 tiles are below this part's threshold")
    _, _, x, h, sc = _problem(width, False)
    umnn_amd.set_forward_precision(mode)
    got, names = _run(_spec(width, False, dev), _t(x, dev), _t(h, dev), _t(sc, dev), 100, False)
    assert all("PIPE" in nm and "P=2" in nm for nm in names), names
    want = _gpu(width, False, 100, False, mode, 1)[0]
    for k in want:
        assert np.array_equal(got[k], want[k]), k


def _tile_integrals(group, tile):
    q = 32 * group + 16 * tile + np.arange(16)
    return q // D, q % D


@pytest.mark.parametrize("tile", [0, 1])
@pytest.mark.parametrize("pipe", [1, 0])
@pytest.mark.parametrize("width", list(HIDDEN))
def test_overflow_in_one_tile_of_a_wave(width, pipe, tile, dev, opts, restore_precision):
    """The embedding of the sixteen integrals of ONE point tile of one wave (tile 0, and mirrored: tile 1) is scaled until the second
    hidden layer leaves fp16's range.  In the paired register only that tile's lane groups turn NaN; the overflow protocol then defers
    the tile GROUP (both tiles of the wave share one marker decision, cc_fwd_shared.h) to the queued bf16 build: the group's 32
    integrals hold a bf16x3 launch's numbers bit for bit, every other integral -- the neighbouring groups included -- the numbers of
    an fp16-piece launch that never saw the overflowing tile.  Through the one-pass log-likelihood too: z likewise, the deferred
    group counted exactly once towards its rows (ll finite, equal to the sum of the published log_jac and z, the same bits on a
    second call: the arrival counters are zero again)."""
    import umnn_amd
    Ws, bs, x, h, sc = _problem(width, False)
    group = 700
    rows, cols = _tile_integrals(group, tile)
    hs = h.reshape(B, E, D).copy()
    hs[rows, :, cols] *= 3e6
    hs = hs.reshape(B, E * D)
    # the overflow is real: |pre-activation| of hidden layer 2 at node 0 (t = x) beyond 65504 for every integral of the tile
    net = O.Net(Ws, bs, O.LEAKY, O.ELU1)
    pre2 = O.mlp_rows(net, O.rows_from(x, hs, D), keep=True)[1][1].reshape(B, D, -1)
    others = np.ones((B, D), bool)
    others[rows, cols] = False
    assert np.all(np.abs(pre2[rows, cols]).max(-1) > 65504) and np.abs(pre2).max(-1)[others].max() < 65504
    spec = _spec(width, False, dev)
    xg, scg = _t(x, dev), _t(sc, dev)
    opts(fwd_pipe=pipe, fwd_p=2, fwd_ns=1)
    n = 100
    umnn_amd.set_forward_precision("bf16x3")
    ob = _run(spec, xg, _t(hs, dev), scg, n, False)[0]
    umnn_amd.set_forward_precision("f16x3")
    of, names = _run(spec, xg, _t(hs, dev), scg, n, False)
    assert all(nm.startswith("cc_fwd_f16<") and ("PIPE" in nm) == bool(pipe) for nm in names), names
    again = _run(spec, xg, _t(hs, dev), scg, n, False)[0]
    clean = _gpu(width, False, n, False, "f16x3", pipe)[0]
    in_group = np.zeros(B * D, bool)
    in_group[32 * group:32 * group + 32] = True
    in_group = in_group.reshape(B, D)
    for k in ("F", "fx", "fx0", "z", "lj", "z_ll"):
        assert np.all(np.isfinite(of[k])), k
        assert np.array_equal(of[k][in_group], ob[k][in_group]), (k, "deferred group: the bf16 build's bits")
        assert np.array_equal(of[k][~in_group], clean[k][~in_group]), (k, "everything else: the fp16-piece launch's bits")
    assert not np.array_equal(ob["F"][~in_group], clean["F"][~in_group]), "the two arithmetics differ somewhere"
    touched = np.unique(np.nonzero(in_group)[0])
    assert np.all(np.isfinite(of["ll"]))
    assert np.array_equal(np.delete(of["ll"], touched), np.delete(clean["ll"], touched))
    ll_host = of["lj"].astype(np.float64).sum(1) - 0.5 * (np.log(2 * np.pi) + of["z"].astype(np.float64) ** 2).sum(1)
    assert U.rel_err(of["ll"][touched], ll_host[touched]) < TOL
    for k in of:
        assert np.array_equal(of[k], again[k]), (k, "second call")


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("width", list(HIDDEN))
def test_results_do_not_depend_on_what_ran_before(width, mode, dev):
    """Identical bits whatever used the registers, LDS and caches before (the paired registers start from zero in every wave)."""
    import umnn_amd
    from umnn_amd import integral as I, IntegrandNetwork
    from umnn_amd.nets import mlp_spec
    ref = _gpu(width, False, 100, False, mode, 1)[0]
    for trial in range(3):
        junk = torch.randn(3000, 3000, device=dev) * (10.0 ** trial)
        (junk @ junk).sum().item()
        wide = IntegrandNetwork(3, 11, [100] * 4, 1).to(dev)
        I.hip_forward(mlp_spec(wide), None, torch.randn(3000, 3, device=dev) * 30, torch.randn(3000, 30, device=dev) * 30, 20)
        out = _gpu.__wrapped__(width, False, 100, False, mode, 1)[0]
        for k in ref:
            assert np.array_equal(out[k], ref[k]), (k, trial)
