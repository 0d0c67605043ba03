"""Drop-in check: what the REFERENCE's own test scripts, its MonotonicMLP.py (BASELINE config C0), ToyExperiments.py (C1)
and TrainVaeFlow.py's flow prior (C4) do with the UMNN classes, done with this package through the `compat/models` import
shim, on the CPU.  Where the reference computed something, tests/golden/g9_dropin.npz holds its inputs and outputs
(tests/golden/make_dropin_golden.py: parameters are set from their names by ``seeded_parameters``, buffers and parameter
gradients are pinned by ``fingerprint``); where its scripts check a known answer, the same answer is checked here."""
import importlib
import os
import sys
import types

import numpy as np
import pytest
import torch

from tests.golden.make_dropin_golden import fingerprint, seeded_parameters

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COMPAT = os.path.join(ROOT, "compat")


@pytest.fixture(scope="module")
def shim():
    """The names the reference's scripts import, resolved through the shim: ``from models.UMNN import ...`` first (importing
    a submodule below rebinds its name in the package, as it would in the reference), then the submodules' classes."""
    sys.path.insert(0, COMPAT)
    try:
        pkg = importlib.import_module("models.UMNN")
        names = {n: getattr(pkg, n) for n in ("UMNNMAFFlow", "MonotonicNN")}
        for mod, n in (("UMNNMAF", "IntegrandNetwork"), ("UMNNMAF", "EmbeddingNetwork"), ("UMNNMAF", "UMNNMAF"),
                       ("NeuralIntegral", "NeuralIntegral"), ("ParallelNeuralIntegral", "ParallelNeuralIntegral")):
            names[n] = getattr(importlib.import_module("models.UMNN." + mod), n)
    finally:
        sys.path.remove(COMPAT)
    assert pkg.__file__.startswith(COMPAT) and all(isinstance(v, type) for v in names.values())
    return types.SimpleNamespace(**names)


@pytest.fixture(scope="module")
def G(golden_dir):
    return dict(np.load(os.path.join(golden_dir, "g9_dropin.npz")))


def _t(a, **kw):
    return torch.from_numpy(np.array(a)).requires_grad_(kw.get("grad", False))


def _names(G, prefix, kind):
    p = f"{prefix}.{kind}."
    return {k[len(p):] for k in G if k.startswith(p)}


def _close(got, want, rtol, what):
    got = got.detach().numpy() if torch.is_tensor(got) else got
    scale = max(float(np.abs(want).max()), 1e-6)
    err = float(np.abs(got - want).max()) / scale
    assert got.shape == want.shape and err <= rtol, (what, err)


def _grads(module):
    return {n: p.grad for n, p in module.named_parameters() if p.grad is not None}


def _buffers_match(module, G, prefix):
    """The buffers construction gave ``module`` (MADE masks ...) are the reference's."""
    bufs = dict(module.named_buffers())
    assert set(bufs) == _names(G, prefix, "buf")
    for n, b in bufs.items():
        assert np.allclose(fingerprint(b, n), G[f"{prefix}.buf.{n}"], rtol=1e-9, atol=1e-9), n


def _grads_match(module, G, prefix, rtol):
    """Every parameter gradient against the reference's, to rtol of its largest entry (max |g| and the components along the
    generator's seeded unit directions)."""
    g = _grads(module)
    assert set(g) == _names(G, prefix, "grad")
    for n, v in g.items():
        want = G[f"{prefix}.grad.{n}"]
        err = float(np.abs(fingerprint(v, n) - want).max())
        assert err <= rtol * max(want[0], 1e-6), (prefix, n, err)


def test_reference_test_jit_passes_against_this_package(tmp_path, shim, G):
    """tests/test_jit.py of the reference: both operators' forward + backward on a 5-net integrand, the full UMNN-MAF block
    (forward, backward reaching every parameter, compute_ll), torch.jit.script / trace of the integrand network matching
    eager mode at two batch sizes, and a traced network saved and loaded -- values against the reference's own."""
    M = shim
    NI, PNI = shim.NeuralIntegral, shim.ParallelNeuralIntegral
    integ = seeded_parameters(M.IntegrandNetwork(nnets=5, nin=2, hidden_sizes=[50, 50], nout=1, device="cpu"))
    x, h = _t(G["jit_int.x"]), _t(G["jit_int.h"])
    flat = torch.cat([p.contiguous().view(-1) for p in integ.parameters()])
    for tag, op in (("ni", lambda *a: NI.apply(*a)), ("pni", lambda *a: PNI.apply(*a, False))):
        integ.zero_grad()
        x0r, xr, hr = torch.zeros(10, 5, requires_grad=True), x.clone().requires_grad_(), h.clone().requires_grad_()
        res = op(x0r, xr, integ, flat, hr, 20)
        res.sum().backward()
        for k, v in (("out", res), ("x0_grad", x0r.grad), ("x_grad", xr.grad), ("h_grad", hr.grad)):
            _close(v, G[f"jit_int.{tag}.{k}"], 1e-5, (tag, k))
        assert len(_grads(integ)) == len(list(integ.parameters()))
        _grads_match(integ, G, f"jit_int.{tag}", 1e-4)
    model = M.UMNNMAF(net=M.EmbeddingNetwork(10, [50, 50], [50, 50], out_made=1, cond_in=0, device="cpu"), input_size=10,
                      nb_steps=20, device="cpu", solver="CCParallel")
    seeded_parameters(model)
    _buffers_match(model, G, "jit_maf")
    xr = _t(G["jit_maf.x"], grad=True)
    z = model(xr)
    z.sum().backward()
    _close(z, G["jit_maf.z"], 1e-5, "z")
    _close(xr.grad, G["jit_maf.x_grad"], 1e-4, "x.grad")
    _grads_match(model, G, "jit_maf", 1e-4)
    ll, zl = model.compute_ll(_t(G["jit_maf.x"]))
    _close(ll, G["jit_maf.ll"], 1e-5, "ll")
    _close(zl, G["jit_maf.ll_z"], 1e-5, "ll z")
    integ.eval()
    scripted = torch.jit.script(integ)
    with torch.no_grad():
        eager = integ(x, h)
        _close(eager, G["jit_int.eval_out"], 1e-6, "integrand")
        assert torch.allclose(scripted(x, h), eager, atol=1e-6)
        traced = torch.jit.trace(integ, (x, h))
        torch.jit.save(traced, str(tmp_path / "integrand_traced.pt"))
        loaded = torch.jit.load(str(tmp_path / "integrand_traced.pt"))
        assert torch.allclose(loaded(x, h), eager, atol=1e-6)
        x2, h2 = torch.randn(37, 5), torch.randn(37, 5)
        assert torch.allclose(traced(x2, h2), integ(x2, h2), atol=1e-6)


def test_reference_numerical_validation_passes_against_this_package(shim):
    """tests/test_numerical_validation.py of the reference, its four known answers: convergence of the quadrature to
    int_0^2 (1 + x^2) = 14/3 (error < 1e-4 at 200 steps), gradients of the integral (d/dx = f(x), d/dx0 = -f(x0)), fitting
    y = x^3 on [0, 2] with an ELU integrand (MSE < 0.1 after 200 Adam steps), and four integrands with closed forms."""
    PNI, M = shim.ParallelNeuralIntegral, shim

    class Fn(torch.nn.Module):
        def __init__(self, f):
            super().__init__()
            self.f = f

        def forward(self, x, h):
            return self.f(x, h)

    def integral(f, a, b, n, batch=1):
        with torch.no_grad():
            return PNI.apply(torch.full((batch, 1), a), torch.full((batch, 1), b), Fn(f), torch.tensor([]),
                             torch.zeros(batch, 1), n, False)
    # integral_convergence
    errs = [abs(integral(lambda x, h: 1 + x ** 2, 0.0, 2.0, n, 5).mean().item() - 14 / 3) for n in (5, 10, 20, 50, 100, 200)]
    assert errs[-1] < 1e-4 and errs[-1] <= errs[0], errs
    # gradient_correctness
    torch.manual_seed(42)
    integ = M.IntegrandNetwork(nnets=3, nin=2, hidden_sizes=[20, 20], nout=1, device="cpu")
    flat = torch.cat([p.contiguous().view(-1) for p in integ.parameters()])
    x0 = torch.zeros(10, 3, requires_grad=True)
    x = torch.randn(10, 3, requires_grad=True)
    h = torch.randn(10, 3, requires_grad=True)
    PNI.apply(x0, x, integ, flat, h, 20, False).sum().backward()
    with torch.no_grad():
        f_x, f_x0 = integ(x, h), integ(x0, h)
    assert torch.allclose(x.grad, f_x, rtol=1e-5, atol=1e-6) and torch.allclose(x0.grad, -f_x0, rtol=1e-5, atol=1e-6)
    assert h.grad is not None and torch.isfinite(h.grad).all()
    # monotonic_fitting
    torch.manual_seed(42)
    xs = torch.linspace(0, 2, 100).reshape(-1, 1)
    integ = M.IntegrandNetwork(nnets=1, nin=2, hidden_sizes=[32, 32], nout=1, act_func="ELU", device="cpu")
    opt = torch.optim.Adam(integ.parameters(), lr=0.01)
    for _ in range(200):
        opt.zero_grad()
        flat = torch.cat([p.contiguous().view(-1) for p in integ.parameters()])
        loss = ((PNI.apply(torch.zeros(100, 1), xs, integ, flat, torch.zeros(100, 1), 30, False) - xs ** 3) ** 2).mean()
        loss.backward()
        opt.step()
    assert loss.item() < 0.1, loss.item()
    # integral_accuracy
    for f, F, a, b in ((lambda x, h: torch.ones_like(x) * 2.0, lambda a, b: 2.0 * (b - a), 0.0, 3.0),
                       (lambda x, h: x, lambda a, b: (b ** 2 - a ** 2) / 2, 0.0, 2.0),
                       (lambda x, h: x ** 2, lambda a, b: (b ** 3 - a ** 3) / 3, 1.0, 3.0),
                       (lambda x, h: torch.exp(x), lambda a, b: np.exp(b) - np.exp(a), 0.0, 1.0)):
        assert abs(integral(f, a, b, 100).item() - F(a, b)) < 1e-3


def test_reference_monotonic_mlp_script_runs_unchanged(shim, G):
    """MonotonicMLP.py's model through `from models.UMNN import MonotonicNN`: the reference's outputs on its test grid and
    on a training batch, the gradient of the script's loss, one epoch of the script's training loop (300 samples, batches
    of 100, Adam 1e-3), and the result monotonic in x_1 on the grid."""
    torch.manual_seed(0)
    mono = seeded_parameters(shim.MonotonicNN(3, [100, 100, 100], nb_steps=100, dev="cpu"))
    xg = _t(G["mono.x_grid"])
    with torch.no_grad():
        _close(mono(xg, torch.zeros(xg.shape[0], 2))[:, 0], G["mono.y_grid"], 1e-5, "grid")
    xb, yb = _t(G["mono.x_batch"]), _t(G["mono.y_batch"])
    y_pred = mono(xb[:, [0]], xb[:, 1:])[:, 0]
    _close(y_pred, G["mono.y_pred"], 1e-5, "batch")
    ((y_pred - yb) ** 2).sum().backward()
    assert len(_grads(mono)) == len(list(mono.parameters()))
    _grads_match(mono, G, "mono", 1e-4)
    opt = torch.optim.Adam(mono.parameters(), 1e-3, weight_decay=1e-5)
    tx = torch.randn(300, 3)
    ty = .001 * (tx[:, 0] ** 3 + tx[:, 0]) + tx[:, 1] ** 2 + torch.sin(tx[:, 2])
    for i in range(0, 300 - 100, 100):
        x = tx[i:i + 100].requires_grad_()
        loss = ((mono(x[:, [0]], x[:, 1:])[:, 0] - ty[i:i + 100]) ** 2).sum()
        opt.zero_grad()
        loss.backward()
        opt.step()
        assert torch.isfinite(loss)
    with torch.no_grad():
        y = mono(xg, torch.zeros(xg.shape[0], 2))[:, 0]
    assert torch.isfinite(y).all() and bool((y[1:] >= y[:-1]).all())


def test_reference_toy_experiment_runs_and_checkpoint_loads_into_the_reference(tmp_path, shim, G):
    """ToyExperiments.py's flow (moons, C1) through `from models import UMNNMAFFlow`: on the generator's weights, the
    reference's masks and log-likelihood; a few training steps on two-moons data, sampling through invert (what the
    script's plot does), and the checkpoint this package writes holds exactly the reference's parameter names and shapes
    (so it loads strictly into the reference's UMNNMAFFlow) and reloads to the same log-likelihood."""
    kw = dict(nb_flow=1, nb_in=2, hidden_derivative=[100] * 4, hidden_embedding=[100] * 4, embedding_s=10, nb_steps=20)
    model = seeded_parameters(shim.UMNNMAFFlow(**kw))
    _buffers_match(model, G, "toy")
    x = _t(G["toy.x"])
    with torch.no_grad():
        ll, z = model.compute_ll(x)
    _close(ll, G["toy.ll"], 1e-5, "ll")
    _close(z, G["toy.z"], 1e-5, "z")
    rng = np.random.RandomState(0)
    t = rng.uniform(0, np.pi, 256)
    moons = np.concatenate([np.stack([np.cos(t[:128]), np.sin(t[:128])], 1),
                            np.stack([1 - np.cos(t[128:]), 0.5 - np.sin(t[128:])], 1)]) + 0.05 * rng.randn(256, 2)
    data = torch.from_numpy(moons.astype(np.float32))
    opt = torch.optim.Adam(model.parameters(), 1e-3, weight_decay=1e-5)
    for i in range(0, 256, 64):
        loss = -model.compute_ll(data[i:i + 64])[0].mean()
        opt.zero_grad()
        loss.backward()
        opt.step()
        assert torch.isfinite(loss)
    with torch.no_grad():
        zs = torch.randn(50, 2)
        xs = model.invert(zs)
        assert torch.isfinite(xs).all()
        assert torch.allclose(model.compute_ll(xs)[1], zs, atol=1e-3)
    torch.save(model.state_dict(), str(tmp_path / "model.pt"))
    sd = torch.load(str(tmp_path / "model.pt"))
    assert [f"{k}:{tuple(v.shape)}" for k, v in sd.items()] == list(G["toy.checkpoint"])
    again = shim.UMNNMAFFlow(**kw)
    again.load_state_dict(sd, strict=True)
    with torch.no_grad():
        assert torch.equal(again.compute_ll(x)[0], model.compute_ll(x)[0])


@pytest.mark.parametrize("solver", ["CC", "CCParallel"])
def test_reference_vae_flow_prior_uses_this_package_and_matches_the_reference(shim, G, solver):
    """BASELINE config C4's caller: TrainVaeFlow.py's MMAVAE builds its conditional UMNNMAFFlow through `from models import
    UMNNMAFFlow` (flows.py:16,309: nb_flow=2, nb_in=z_size=8, cond_in=h_size=16) and calls compute_log_jac_bis and
    forceLipshitz (flows.py:318-330).  Through the shim, on the generator's weights and noise: z_k, log|det J|, the gradients
    of a loss of both (every parameter, z_0, the context) and the parameters after forceLipshitz(1.5) match the reference."""
    p = f"vae_{solver}"
    flow = shim.UMNNMAFFlow(nb_flow=2, nb_in=8, hidden_derivative=[50] * 4, hidden_embedding=[32, 32], embedding_s=6,
                                nb_steps=20, solver=solver, cond_in=16, device="cpu")
    assert type(flow).__module__.startswith("umnn_amd")
    seeded_parameters(flow)
    _buffers_match(flow, G, p)
    z0, hc = _t(G[f"{p}.z0"], grad=True), _t(G[f"{p}.h"], grad=True)
    zk, ldj = flow.compute_log_jac_bis(z0, hc)
    (zk.pow(2).sum() - ldj.sum()).backward()
    _close(zk, G[f"{p}.zk"], 1e-4, "zk")
    _close(ldj, G[f"{p}.ldj"], 1e-4, "ldj")
    _close(z0.grad, G[f"{p}.z0_grad"], 2e-4, "z0.grad")
    _close(hc.grad, G[f"{p}.h_grad"], 2e-4, "h.grad")
    _grads_match(flow, G, p, 2e-4)
    before = {n: v.detach().clone() for n, v in flow.named_parameters()}
    torch.manual_seed(5)                # the generator's seed: the spectral-norm estimate starts from torch.randn
    flow.forceLipshitz(1.5)
    after = dict(flow.named_parameters())
    assert set(after) == _names(G, p, "divisor")
    for n, v in after.items():          # the reference divided each parameter by one scalar: the same division here
        assert torch.allclose(v.detach(), before[n] / float(G[f"{p}.divisor.{n}"]), rtol=1e-5, atol=1e-6), n
