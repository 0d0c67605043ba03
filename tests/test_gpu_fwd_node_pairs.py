"""The node-paired ring of the pipelined two-tile forward loop (fp16 pieces, merged layout: hidden widths 48..51, three or more
hidden layers; umnn_amd/csrc/cc_fwd_bf16_kernel.h, NODE_PAIRS): two nodes of each point tile in flight, a layer's weight fragments
read once per four tile-nodes.  Per tile-node the operations and their order are those of the one-node loop, and the output stage
runs per node in node order, so every output keeps its bits: the yardstick is the plain loop (fwd_pipe = 0), which this change does
not touch.

Shapes are small on purpose: 23 x 7 = 161 integrals = 6 tile groups of 32 (two workgroups; the last group holds ONE integral: a
partly filled tile and a dead one).  A 60-wide net (LIVE = 0, 24-slot plan) and two-hidden-layer nets stay on the one-node loop and
run as controls.

Node ranges: a wave's range [k_lo, k_hi) = [part (n+1) / ns, (part+1) (n+1) / ns) runs its pairs first and a leftover node through the
one-node body.  fwd_ns accepts 1, 2 and 4 (the waves of a workgroup: 3 is not an option value), so the cases are n + 1 in
{2, 3, 4, 5, 7, 8} x ns in {1, 2, 4} (a split into more parts than nodes runs unsplit):
    a range of a single node            5 nodes / 4: [0,1) [1,2) [2,3) [3,5);  3 / 2: [0,1) [1,3);  7 / 4: [0,1) ...
    ranges that start at an odd k       7 / 2: [0,3) [3,7);  5 / 4: [1,2) [3,5);  3 / 2: [1,3)
    node 0 first of a pair              every ns = 1 case, 8 / 4: [0,2)
    node n second of a pair             n + 1 = 2;  4 / 1;  8 / 4: [6,8);  3 / 2: [1,3)
    node n the leftover behind pairs    n + 1 = 3, 5, 7 at ns = 1;  5 / 2: [2,5) = pair (2,3) + node 4
    a leftover that is not node n       7 / 2: [0,3) = pair (0,1) + node 2

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

E = 30
SHAPE = (23, 7)
PAIRED = "cc_fwd_f16<T=4,PARTS=2,P=2,EXACT=1,LIVE=13,PIPE>"


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _t(a, dev):
    return torch.from_numpy(np.array(a)).to(dev)            # (a copy: the shared arrays are read-only)


def _kname():
    from umnn_amd import _lib
    return _lib.lib().umnn_last_kernel_name().decode()


@functools.lru_cache(maxsize=None)
def _problem(width, nh, relu, shape=SHAPE):
    """Weights and inputs of one integrand (host arrays, shared, never modified).  Weights as torch.nn.Linear draws them, uniform in
    +-1/sqrt(fan_in): see tests/test_gpu_fwd_paired_output.py for why (the conditioning of the two-piece modes is not this file's
    subject)."""
    B, D = shape
    rng = np.random.RandomState(7000 + 16 * width + 2 * nh + relu + 1000 * B)
    sizes = [1 + E] + [width] * nh + [1]
    Ws = [rng.uniform(-1, 1, (sizes[i + 1], sizes[i])).astype(np.float32) / np.float32(np.sqrt(sizes[i])) for i in range(len(sizes) - 1)]
    bs = [rng.uniform(-1, 1, sizes[i + 1]).astype(np.float32) / np.float32(np.sqrt(sizes[i])) for i in range(len(sizes) - 1)]
    x = (rng.randn(B, D) * 2).astype(np.float32)
    h = rng.randn(B, E * D).astype(np.float32)
    sc = np.linspace(-0.3, 0.4, D).astype(np.float32)
    for a in Ws + bs + [x, h, sc]:
        a.setflags(write=False)
    return Ws, bs, x, h, sc


def _spec(width, nh, relu, sigmoid, dev, shape=SHAPE):
    from umnn_amd import _lib
    from umnn_amd.nets import MlpSpec
    Ws, bs = _problem(width, nh, relu, shape)[:2]
    lin = []
    for W, b in zip(Ws, bs):
        m = torch.nn.Linear(W.shape[1], W.shape[0])
        with torch.no_grad():
            m.weight.copy_(torch.from_numpy(W.copy()))
            m.bias.copy_(torch.from_numpy(b.copy()))
        lin.append(m.to(dev))
    return MlpSpec(lin, _lib.ACT_RELU if relu else _lib.ACT_LEAKY_RELU, _lib.OUT_SIGMOID if sigmoid else _lib.OUT_ELU_PLUS_ONE)


def _run(spec, x, h, sc, n, inv_f):
    """Every output the forward kernel writes: F, f(x), f(x0) from the quadrature entry point; z, log_jac from the flow-block entry
    point and ll (with its z) from the one-pass log-likelihood (plain integrand only).  -> (dict of host arrays, kernel names)."""
    from umnn_amd import integral as I
    out, names = {}, []
    F, fx, fx0 = I.hip_forward(spec, None, x, h, n, inv_f=inv_f)
    names.append(_kname())
    out.update(F=F, fx=fx, fx0=fx0)
    if not inv_f:
        z, lj = I.hip_flow_block(spec, x, h, sc, n)[:2]
        names.append(_kname())
        ll = torch.empty(x.shape[0], device=x.device, dtype=torch.float32)
        scratch = torch.empty_like(x)
        z1 = I.hip_flow_ll_block(spec, x, h, sc, n, False, True, True, ll, scratch)
        names.append(_kname())
        out.update(z=z, lj=lj, ll=ll, z_ll=z1)
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in out.items()}, names


def _launch(width, nh, relu, sigmoid, n, inv_f, mode, pipe, ns, shape=SHAPE, h=None):
    """One case on the GPU with two tiles per wave; fwd_p, fwd_pipe, fwd_ns and the precision saved and restored."""
    import umnn_amd
    from umnn_amd import _lib
    dev = torch.device("cuda:0")
    _, _, x, h0, sc = _problem(width, nh, relu, shape)
    old = umnn_amd.get_forward_precision()
    saved = {k: _lib.get_option(k) for k in ("fwd_pipe", "fwd_p", "fwd_ns")}
    try:
        umnn_amd.set_forward_precision(mode)
        _lib.set_option("fwd_pipe", pipe)
        _lib.set_option("fwd_p", 2)
        _lib.set_option("fwd_ns", ns)
        return _run(_spec(width, nh, relu, sigmoid, dev, shape), _t(x, dev), _t(h0 if h is None else h, dev), _t(sc, dev), n, inv_f)
    finally:
        umnn_amd.set_forward_precision(old)
        for k, v in saved.items():
            _lib.set_option(k, v)


_gpu = functools.lru_cache(maxsize=None)(_launch)


def _same_bits(piped, plain, inv_f):
    assert set(piped) == set(plain) and len(piped) == (3 if inv_f else 7)
    for k in piped:
        assert np.array_equal(piped[k], plain[k], equal_nan=True), k
    if not inv_f:
        assert np.array_equal(piped["z"], piped["z_ll"])


NETS = [(w, nh, relu, sig, inv_f) for w in (48, 50, 51, 60) for nh in (2, 3, 4) for relu in (False, True)
        for sig in (False, True) for inv_f in (False, True)]
NET_IDS = [f"w{w}-h{nh}-{'relu' if relu else 'leaky'}-{'sigmoid' if sig else 'elu1'}-{'invf' if inv_f else 'f'}" for w, nh, relu, sig, inv_f in NETS]


@pytest.mark.parametrize("width,nh,relu,sigmoid,inv_f", NETS, ids=NET_IDS)
def test_ring_and_plain_loop_agree_bit_for_bit(width, nh, relu, sigmoid, inv_f, dev):
    """fwd_pipe = 1 against fwd_pipe = 0 under f16x3, seven nodes (three pairs and a leftover): F, f(x), f(x0), z, log_jac and the
    one-pass ll with its z.  Widths 48, 50, 51 run the ring from three hidden layers on; the 60-wide net is the control."""
    piped, names1 = _gpu(width, nh, relu, sigmoid, 6, inv_f, "f16x3", 1, 1)
    plain, names0 = _gpu(width, nh, relu, sigmoid, 6, inv_f, "f16x3", 0, 1)
    assert all(nm.startswith("cc_fwd_f16<") and "PIPE" in nm and "P=2" in nm and ("LIVE=13" in nm) == (width != 60) for nm in names1), names1
    assert all(nm.startswith("cc_fwd_f16<") and "PIPE" not in nm and "P=2" in nm for nm in names0), names0
    _same_bits(piped, plain, inv_f)


NODES = [(n1 - 1, ns) for n1 in (2, 3, 4, 5, 7, 8) for ns in (1, 2, 4)] + [(100, 1)]


@pytest.mark.parametrize("nh", [3, 4])
@pytest.mark.parametrize("n,ns", NODES, ids=[f"nodes{n + 1}-ns{ns}" for n, ns in NODES])
def test_node_counts_and_range_parities(n, ns, nh, dev):
    """Every length and starting parity of a wave's node range (table in the module docstring): the ring with its leftover body
    against the plain loop under the same split, bit for bit."""
    piped, names = _gpu(50, nh, False, False, n, False, "f16x3", 1, ns)
    plain = _gpu(50, nh, False, False, n, False, "f16x3", 0, ns)[0]
    assert all(nm == PAIRED for nm in names), names
    _same_bits(piped, plain, False)
    # the split itself only regroups the quadrature sum: f(x) and f(x0) are single nodes and keep their bits across ns
    whole = _gpu(50, nh, False, False, n, False, "f16x3", 1, 1)[0]
    assert np.array_equal(piped["fx"], whole["fx"]) and np.array_equal(piped["fx0"], whole["fx0"])
    assert U.rel_err(piped["F"], whole["F"]) < TOL


@pytest.mark.parametrize("ns", [1, 2])
@pytest.mark.parametrize("shape", [(5, 7), (37, 3)], ids=["5x7", "37x3"])
def test_ragged_tiles(shape, ns, dev):
    """5 x 7 = 35 integrals: a full pair of tiles, then a wave with three live lanes in tile 0 and a dead tile 1.  37 x 3 = 111: the
    last wave has a full tile 0 and fifteen lanes of tile 1."""
    B, D = shape
    Ws, bs, x, h, sc = _problem(50, 4, False, shape)
    piped, names = _gpu(50, 4, False, False, 6, False, "f16x3", 1, ns, shape)
    plain = _gpu(50, 4, False, False, 6, False, "f16x3", 0, ns, shape)[0]
    assert all(nm == PAIRED for nm in names), names
    _same_bits(piped, plain, False)
    net = O.Net(Ws, bs, O.LEAKY, O.ELU1)
    F = O.integrate_parallel(net, np.zeros_like(x), x, h, 6)
    for k, ref in (("F", F), ("fx", O.integrand(net, x, h)), ("fx0", O.integrand(net, np.zeros_like(x), h))):
        assert piped[k].shape == (B, D) and U.rel_err(piped[k], ref) < TOL, k


@functools.lru_cache(maxsize=None)
def _oracle(width, nh, relu, sigmoid, n, inv_f):
    Ws, bs, x, h, sc = _problem(width, nh, relu)
    B, D = SHAPE
    net = O.Net(Ws, bs, O.RELU if relu else O.LEAKY, O.SIGMOID if sigmoid else O.ELU1)
    x0 = np.zeros_like(x)
    ref = {"F": O.integrate_parallel(net, x0, x, h, n, inv_f=inv_f), "fx": O.integrand(net, x, h), "fx0": O.integrand(net, x0, h)}
    if not inv_f:
        ref["z"] = np.exp(sc)[None, :] * (ref["F"] + h.reshape(B, -1, D)[:, 0, :])
        ref["lj"] = np.log(ref["fx"] + np.float32(1e-10)) + sc[None, :]
        ref["ll"] = ref["lj"].sum(1) + np.float32(-.5) * (np.log(np.float32(np.pi) * np.float32(2)) + ref["z"] ** 2).sum(1)
    return ref


ORACLE = [(w, nh, relu, sig, n, inv_f) for (w, nh) in ((48, 3), (50, 3), (50, 4), (51, 4)) for relu, sig in ((False, False), (True, True))
          for n in (7, 100) for inv_f in (False, True)]


@pytest.mark.parametrize("width,nh,relu,sigmoid,n,inv_f", ORACLE,
                         ids=[f"w{w}-h{nh}-{'relu-sigmoid' if r else 'leaky-elu1'}-n{n}-{'invf' if i else 'f'}" for w, nh, r, s, n, i in ORACLE])
def test_ring_against_oracle(width, nh, relu, sigmoid, n, inv_f, dev):
    """The quadrature, flow-block and one-pass log-likelihood entry points against the oracle, at the tolerance of
    tests/test_gpu_forward.py.  n = 7: eight nodes, pairs only; n = 100: fifty pairs and the leftover node n."""
    ref = _oracle(width, nh, relu, sigmoid, n, inv_f)
    got, names = _gpu(width, nh, relu, sigmoid, n, inv_f, "f16x3", 1, 1)
    assert all(nm == PAIRED for nm in names), names
    for k in ("F", "fx", "fx0") + (() if inv_f else ("z", "ll")):
        err = U.rel_err(got[k], ref[k])
        print(f"{k}: rel err {err:.3e}")
        assert err < TOL, (k, err)
    if not inv_f:
        assert np.all(np.abs(got["lj"] - ref["lj"]) <= TOL * np.maximum(1.0, np.abs(ref["lj"])))


@pytest.mark.parametrize("nh", [3, 4])
def test_planner_names_the_paired_variant(nh, dev):
    """At these options the launch note still names the PIPE / LIVE=13 / P=2 variant (no new kernel name), every entry point; and
    the bf16 build of the same name -- the queued overflow fallback -- agrees with its own plain loop as before."""
    names = _gpu(50, nh, False, False, 6, False, "f16x3", 1, 1)[1]
    assert names == [PAIRED] * 3, names
    piped, names_b = _gpu(50, nh, False, False, 6, False, "bf16x3", 1, 1)
    assert names_b == [PAIRED.replace("cc_fwd_f16<", "cc_fwd_bf16<")] * 3, names_b
    _same_bits(piped, _gpu(50, nh, False, False, 6, False, "bf16x3", 0, 1)[0], False)


def _tile_integrals(group, tile):
    q = 32 * group + 16 * tile + np.arange(16)
    return q // SHAPE[1], q % SHAPE[1]


@pytest.mark.parametrize("tile", [0, 1])
@pytest.mark.parametrize("nh", [3, 4])
def test_overflow_in_one_tile_of_a_wave(nh, tile, dev):
    """Inputs as in tests/test_gpu_fwd_paired_output.py::test_overflow_in_one_tile_of_a_wave: the embedding of the sixteen integrals
    of ONE point tile of one wave is scaled until the second hidden layer leaves fp16's range.  Both nodes of a pair of that tile then
    carry NaN through the ring; the group is deferred and comes back with the bits of a bf16x3 run of the same launch; its other tile
    holds what bf16x3 gives it on the unscaled inputs (the overflow next to it changed nothing); every other group keeps the bits of
    an fp16-piece launch that never saw the overflow."""
    B, D = SHAPE
    Ws, bs, x, h, sc = _problem(50, nh, False)
    group, n = 2, 6
    rows, cols = _tile_integrals(group, tile)
    hs = h.reshape(B, E, D).copy()
    hs[rows, :, cols] *= 3e6
    hs = hs.reshape(B, E * D)
    net = O.Net(Ws, bs, O.LEAKY, O.ELU1)
    pre2 = O.mlp_rows(net, O.rows_from(x, hs, D), keep=True)[1][1].reshape(B, D, -1)
    others = np.ones((B, D), bool)
    others[rows, cols] = False
    assert np.all(np.abs(pre2[rows, cols]).max(-1) > 65504) and np.abs(pre2).max(-1)[others].max() < 65504
    ob = _launch(50, nh, False, False, n, False, "bf16x3", 1, 1, h=hs)[0]
    of, names = _launch(50, nh, False, False, n, False, "f16x3", 1, 1, h=hs)
    assert all(nm == PAIRED for nm in names), names
    clean = _gpu(50, nh, False, False, n, False, "f16x3", 1, 1)[0]
    clean_b = _gpu(50, nh, False, False, n, False, "bf16x3", 1, 1)[0]
    in_group = np.zeros(B * D, bool)
    in_group[32 * group:32 * group + 32] = True
    other_tile = np.zeros(B * D, bool)
    other_tile[32 * group + 16 * (1 - tile):32 * group + 16 * (2 - tile)] = True
    in_group, other_tile = in_group.reshape(B, D), other_tile.reshape(B, D)
    for k in ("F", "fx", "fx0", "z", "lj", "z_ll"):
        assert np.all(np.isfinite(of[k])), k
        assert np.array_equal(of[k][in_group], ob[k][in_group]), (k, "deferred group: the bf16 build's bits")
        assert np.array_equal(of[k][other_tile], clean_b[k][other_tile]), (k, "the other tile of the wave: unchanged")
        assert np.array_equal(of[k][~in_group], clean[k][~in_group]), (k, "everything else: the fp16-piece launch's bits")
    assert not np.array_equal(ob["F"][~in_group], clean["F"][~in_group]), "the two arithmetics differ somewhere"
    touched = np.unique(np.nonzero(in_group)[0])
    assert np.all(np.isfinite(of["ll"]))
    assert np.array_equal(np.delete(of["ll"], touched), np.delete(clean["ll"], touched))


@pytest.mark.parametrize("nh", [3, 4])
def test_results_do_not_depend_on_what_ran_before(nh, dev):
    """The same launch after two different preceding launches gives the same bits (pattern of
    tests/test_gpu_fwd_paired_output.py): a vector write into a register that an in-flight MFMA still reads as its C operand shows
    here, as an output that depends on what the registers held."""
    from umnn_amd import integral as I, IntegrandNetwork
    from umnn_amd.nets import mlp_spec
    ref = _gpu(50, nh, False, False, 6, False, "f16x3", 1, 1)[0]
    for trial in range(2):
        if trial == 0:
            junk = torch.randn(2000, 2000, device=dev) * 1e3
            (junk @ junk).sum().item()
        else:
            wide = IntegrandNetwork(3, 11, [100] * 4, 1).to(dev)
            I.hip_forward(mlp_spec(wide), None, torch.randn(3000, 3, device=dev) * 30, torch.randn(3000, 30, device=dev) * 30, 20)
        out = _launch(50, nh, False, False, 6, False, "f16x3", 1, 1)[0]
        for k in ref:
            assert np.array_equal(out[k], ref[k]), (k, trial)
