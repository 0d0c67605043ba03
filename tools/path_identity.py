#!/usr/bin/env python
"""Which path every call takes, and what it computes, as a file that two checkouts can be compared by.

    python tools/path_identity.py run OUT.pt                    (GPU; once per checkout, each in its own process)
    python tools/path_identity.py compare A.pt B.pt [REPORT]    (no GPU)

``run`` executes a fixed list of small cases with fixed seeds -- the smallest shapes that reach each arm of the path selection in
flow.py / integral.py / ops.py -- eagerly and under the compile backends tests/test_gpu_torch_compile.py uses (aot_eager for every
case; Inductor, where Triton is installed, for the two kinds of graph that file compiles with it), and records per case every
output and gradient tensor, ``path_taken()``, ``backward_path_taken()``, ``umnn_last_kernel_name()``, the last kernel of the
backward's main pass (``umnn_last_kernel_name_of(PROF_BACKWARD)``) and the ``umnn_launch_count()`` delta.  The list ends with the
GPU cases of tests/_bwd_plan_cases.py (one ``integral.hip_backward`` call per kernel family and option of the backward's launch plan)
and of tests/_fwd_plan_cases.py (forward, flow block, ll block, bracket search and Newton solves per family and rule of the forward's;
``invert`` bracket / newton / jacobi are further up) and with the conditioner's cases: one ``raw`` call per route of ``MADE`` and
``ConditionnalMADE`` with fp32 and bf16 output, ``raw_rows``, a training step through the one-node chain, the progressive conditioner
of ``invert`` and a ``GraphedLL`` capture with replays; for every case also the conditioner's launch count delta
(``umnn_made_launch_count()``) and last kernel (``umnn_last_made_kernel_name()``).  A case that raises is recorded by its exception
type.  ``compare`` wants ``torch.equal`` on every tensor and equality of every string and count; it prints (and writes to REPORT) the number of tensors, the number of mismatches and
the kernel names seen, and exits non-zero on any mismatch.  Only the public API is used, so the file runs in older checkouts too (with tests/_bwd_plan_cases.py and tests/_fwd_plan_cases.py copied along)."""
import os
import sys
import warnings

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

B = 37      # (the tiles of the forward kernels straddle samples)


def _boost(model):
    with torch.no_grad():
        for m in model.modules():
            if isinstance(m, torch.nn.Linear) and type(m) is torch.nn.Linear:
                m.weight.mul_(1.5)


def _flow(dev, d=3, E=4, hidden=(50, 50, 50, 50), n=20, nb_flow=2, cond_in=0, seed=0):
    import umnn_amd
    torch.manual_seed(seed)
    f = umnn_amd.UMNNMAFFlow(nb_flow=nb_flow, nb_in=d, hidden_derivative=list(hidden), hidden_embedding=[64, 64], embedding_s=E,
                             nb_steps=n, solver="CCParallel", cond_in=cond_in)
    for i in range(nb_flow):
        _boost(f.nets[i].net.parallel_nets)
    return f.to(dev)


def _grads(model, loss, *leaves):
    model.zero_grad()
    loss.backward()
    return [t.grad for t in leaves] + [p.grad for p in model.parameters() if p.grad is not None]


def _x(dev, d, seed=1, rows=B, scale=0.5):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(rows, d, generator=g) * scale).to(dev)


# ---------------------------------------------------------------------------------------------------------------- the cases
# Each: (name, backends, make(dev) -> (model, fn(*tensors) -> tensors, tensors, after(model, outs, tensors) -> more tensors or None)).
# ``fn`` is what gets compiled; ``after`` (the backward) runs outside it, as in the test suite.
def _ll_train(setup=None, rows=B, **flow_kw):
    def make(dev):
        flow = _flow(dev, **flow_kw)
        if setup is not None:
            setup(flow)
        x = _x(dev, flow.nets[0].input_size, rows=rows).requires_grad_()
        return flow, (lambda x: flow.compute_ll(x)), (x,), (lambda flow, out, ts: _grads(flow, -out[0].mean(), *ts))
    return make


def _no_grad(call, **flow_kw):
    def make(dev):
        flow = _flow(dev, **flow_kw)
        x = _x(dev, flow.nets[0].input_size)

        def fn(x):
            with torch.no_grad():
                return call(flow, x)
        return flow, fn, (x,), None
    return make


def _scaling_trains(flow):
    for net in flow.nets:
        net.scaling.requires_grad_(True)


def _with_x0(dev):
    flow = _flow(dev)
    blk = flow.nets[0]
    x, x0 = _x(dev, 3).requires_grad_(), (_x(dev, 3, seed=2) * 0.2).requires_grad_()
    return blk, (lambda x, x0: blk(x, x0=x0)), (x, x0), (lambda m, out, ts: _grads(m, (out * out).sum(), *ts))


def _block_log_jac(dev):
    flow = _flow(dev)
    blk = flow.nets[0]
    x = _x(dev, 3).requires_grad_()
    return blk, (lambda x: blk.compute_log_jac(x)), (x,), (lambda m, out, ts: _grads(m, out.sum(), *ts))


def _captured_ll(dev):
    flow = _flow(dev)
    xs = _x(dev, 3)

    def fn(xs):
        with torch.no_grad():
            side = torch.cuda.Stream(device=dev)
            side.wait_stream(torch.cuda.current_stream(dev))
            with torch.cuda.stream(side):
                flow.compute_ll(xs)
            torch.cuda.current_stream(dev).wait_stream(side)
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph):
                cap = flow.compute_ll(xs)
            graph.replay()
            graph.replay()
            torch.cuda.synchronize()
            return [t.clone() for t in cap]
    return flow, fn, (xs,), None


def _quadrature(op, inv_f):
    def make(dev):
        import umnn_amd
        torch.manual_seed(3)
        d, E = 3, 4
        net = umnn_amd.IntegrandNetwork(d, 1 + E, [50, 50, 50], 1).to(dev)
        _boost(net)
        x0, x, h = (_x(dev, d, seed=4) * 0.2).requires_grad_(), _x(dev, d, seed=5).requires_grad_(), _x(dev, E * d, seed=6).requires_grad_()
        cls = getattr(umnn_amd, op)
        extra = (True,) if inv_f else ()

        def fn(x0, x, h):
            return cls.apply(x0, x, net, umnn_amd.integral._flatten(net.parameters()), h, 20, *extra)

        def after(m, out, ts):
            outs = out if isinstance(out, tuple) else (out,)
            loss = sum((o * torch.linspace(-1, 1, B, device=dev).view(-1, 1) * (k + 1)).sum() for k, o in enumerate(outs))
            return _grads(m, loss, *ts)
        return net, fn, (x0, x, h), after
    return make


def _monotonic(inverse):
    def make(dev):
        import umnn_amd
        torch.manual_seed(7)
        m = umnn_amd.MonotonicNN(3, [50, 50, 50], nb_steps=20).to(dev)
        x, h = _x(dev, 1, seed=8).requires_grad_(), _x(dev, 2, seed=9).requires_grad_()
        fn = (lambda x, h: m.inverse(x, h)) if inverse else (lambda x, h: m(x, h))
        return m, fn, (x, h), (lambda m, out, ts: _grads(m, (out * torch.linspace(-1, 1, B, device=dev).view(-1, 1)).sum(), *ts))
    return make


def _inverse_integral(dev):
    import umnn_amd
    torch.manual_seed(10)
    d, E = 3, 4
    net = umnn_amd.IntegrandNetwork(d, 1 + E, [50, 50, 50], 1).to(dev)
    t, h = _x(dev, d, seed=11).requires_grad_(), _x(dev, E * d, seed=12).requires_grad_()

    def fn(t, h):
        return umnn_amd.InverseNeuralIntegral.apply(t, net, umnn_amd.integral._flatten(net.parameters()), h, 20, (-50., 50.), 1e-6, 64, True)
    return net, fn, (t, h), (lambda m, out, ts: _grads(m, (out[0] * torch.linspace(-1, 1, B, device=dev).view(-1, 1)).sum(), *ts))


def _invert(method, cond):
    def make(dev):
        flow = _flow(dev, cond_in=2 if cond else 0)
        z = _x(dev, 3, seed=13, scale=1.0)
        ctx = _x(dev, 2, seed=14) if cond else None
        kw = dict(iter=4) if method == "bracket" else dict(return_info=True) if method == "jacobi" else {}

        def fn(z):
            out = flow.invert(z, context=ctx, method=method, **kw)
            if method != "jacobi":
                return out
            x, info = out
            return [x] + list(info["status"]) + [torch.tensor(info["sweeps"]), torch.tensor(info["converged"]),
                                                 torch.tensor([e for per_block in info["max_evals"] for e in per_block])]
        return flow, fn, (z,), None
    return make


def _backward_plan_case(c):
    def make(dev):
        from tests import _bwd_plan_cases
        return None, (lambda: _bwd_plan_cases.run(c, dev)), (), None
    return make


def _backward_plan_cases():
    from tests import _bwd_plan_cases
    return [(f"backward plan: {c['id']}", EAGER, _backward_plan_case(c)) for c in _bwd_plan_cases.GPU_CASES]


def _forward_plan_case(c):
    def make(dev):
        from tests import _fwd_plan_cases
        return None, (lambda: _fwd_plan_cases.run(c, dev)), (), None
    return make


def _forward_plan_cases():
    from tests import _fwd_plan_cases
    return [(f"forward plan: {c['id']}", EAGER, _forward_plan_case(c)) for c in _fwd_plan_cases.GPU_CASES]


def _plan_block_case(ll):
    """A flow block through the launch plan's forward cases: the block forward (z, log_jac) or the one-pass log-likelihood"""
    def make(dev):
        flow = _flow(dev, nb_flow=1)
        x = _x(dev, 3)

        def fn(x):
            with torch.no_grad():
                return flow.compute_ll(x) if ll else flow.nets[0].compute_log_jac(x)
        return flow, fn, (x,), None
    return make


def _restore_made_switches():
    """The conditioner's switches as this process started with them: what its environment says (only setters exist in every checkout)."""
    import umnn_amd
    env = os.environ.get
    umnn_amd.set_made_fast_path(env("UMNN_MADE_BF16X3", "1") != "0")
    umnn_amd.set_made_fused(env("UMNN_MADE_FUSED", "1") != "0", max_rows=int(env("UMNN_MADE_FUSED_MAX_ROWS", "32768")),
                            wide_out=env("UMNN_MADE_FUSED_WIDE_OUT", "0") == "1", hybrid=env("UMNN_MADE_FUSED_HYBRID", "0") == "1",
                            layered=env("UMNN_MADE_LAYERED", "1") != "0")


def _conditioner(cond, bf16, rows=B, hidden=(37,), E=30, fast=True, fused=True, call="raw", **fused_kw):
    """One conditioner call (``MADE.raw`` / ``ConditionnalMADE.raw`` / ``raw_rows`` / a training step through ``raw``) under the given
    switches: with E = 30 the output is 600 columns wide (the routes of wide outputs), with E = 3 it is 60 (the one-launch kernel)."""
    def make(dev):
        import umnn_amd
        torch.manual_seed(20)
        nin, c = 20, 12
        if cond:
            net = umnn_amd.ConditionnalMADE(nin, c, list(hidden), (nin + c) * E, num_masks=1, natural_ordering=True).to(dev)
        else:
            net = umnn_amd.MADE(nin, list(hidden), nin * E, num_masks=1, natural_ordering=True).to(dev)
        args = (_x(dev, nin, seed=21, rows=rows),) + ((_x(dev, c, seed=22, rows=rows),) if cond else ())
        if call == "train":
            args = tuple(a.requires_grad_() for a in args)
        sel = torch.arange(7, nin * E, nin, device=dev)

        def fn(*args):
            try:
                umnn_amd.set_made_fast_path(fast)
                umnn_amd.set_made_fused(fused, **fused_kw)
                if call == "train":
                    return net.raw(*args)
                with torch.no_grad():
                    return net.raw_rows(args[0], sel) if call == "raw_rows" else net.raw(*args, out_dtype=torch.bfloat16 if bf16 else None)
            finally:
                _restore_made_switches()
        after = (lambda m, out, ts: _grads(m, (out * out).sum(), *ts)) if call == "train" else None
        return net, fn, args, after
    return make


def _conditioner_cases():
    routes = [("fast path off (F.linear chain)", dict(fast=False)), ("fused off (split + GEMM)", dict(fused=False)),
              ("narrow (one launch)", dict(E=3)), ("wide_out (one launch)", dict(wide_out=True)),
              ("hybrid (hidden stack + GEMM)", dict(hidden=(37, 37), hybrid=True)), ("layered (one launch per layer)", dict()),
              ("layered, 4097 rows (output layer on the library)", dict(rows=4097)), ("layered off (split + GEMM)", dict(layered=False)),
              ("max_rows 16 (split + GEMM)", dict(E=3, max_rows=16)), ("513-wide hidden layer (split + GEMM)", dict(hidden=(513, 16)))]
    cases = [(f"conditioner {'ConditionnalMADE' if cond else 'MADE'} {'bf16' if bf16 else 'fp32'}: {name}", EAGER, _conditioner(cond, bf16, **kw))
             for name, kw in routes for cond in (False, True) for bf16 in (False, True)]
    cases.append(("conditioner MADE.raw_rows (4200-row output layer)", EAGER, _conditioner(False, False, E=210, call="raw_rows")))
    cases += [(f"conditioner {'ConditionnalMADE' if cond else 'MADE'}: training step through the one-node chain", EAGER,
               _conditioner(cond, False, call="train")) for cond in (False, True)]
    return cases


def _progressive_invert(cond):
    def make(dev):
        flow = _flow(dev, cond_in=2 if cond else 0)
        z = _x(dev, 3, seed=13, scale=1.0)
        ctx = _x(dev, 2, seed=14) if cond else None
        return flow, (lambda z: flow.invert(z, context=ctx, method="newton", conditioner="progressive")), (z,), None
    return make


def _graphed_ll(dev):
    import umnn_amd
    flow = _flow(dev)
    xs = _x(dev, 3)

    def fn(xs):
        graphed = umnn_amd.GraphedLL(flow, xs)
        first = [t.clone() for t in graphed(xs)]
        return first + [t.clone() for t in graphed(xs * 0.5)]
    return flow, fn, (xs,), None


EAGER, COMPILED, INDUCTOR = ("eager",), ("eager", "aot_eager"), ("eager", "aot_eager", "inductor")
WIDE_FIRST = dict(d=8, E=10, hidden=(100, 50, 50, 50, 50))           # the z_2 hand-off from the training forward to the backward
DEEP_WIDE = dict(d=2, E=4, hidden=(100, 72, 80, 96, 70), n=10)       # no shape-exact HIP backward: the ATen backward
CASES = [
    ("flow.forward", COMPILED, _no_grad(lambda f, x: f(x))),
    ("flow.compute_ll no_grad (one-pass)", INDUCTOR, _no_grad(lambda f, x: f.compute_ll(x))),
    ("flow.compute_ll train (one node)", COMPILED, _ll_train()),
    ("flow.compute_ll train, bf16 embedding", COMPILED, _ll_train(lambda f: f.set_embedding_dtype(torch.bfloat16))),
    ("flow.compute_ll train, trainable scaling (composed)", COMPILED, _ll_train(_scaling_trains)),
    ("block.forward with x0 (IntegralWithJacobianParams)", COMPILED, _with_x0),
    ("flow.compute_log_jac no_grad", COMPILED, _no_grad(lambda f, x: f.compute_log_jac(x))),
    ("block.compute_log_jac no_grad", COMPILED, _no_grad(lambda f, x: f.nets[0].compute_log_jac(x))),
    ("block.compute_log_jac train", COMPILED, _block_log_jac),
    ("flow.compute_ll in a torch.cuda.graph capture, replayed", EAGER, _captured_ll),
    ("wide-first flow.compute_ll train (z_2 hand-off)", COMPILED, _ll_train(**WIDE_FIRST)),
    ("deep wide flow.compute_ll train (ATen backward)", COMPILED, _ll_train(rows=8, **DEEP_WIDE)),
    ("ParallelNeuralIntegral", COMPILED, _quadrature("ParallelNeuralIntegral", False)),
    ("ParallelNeuralIntegral inv_f", COMPILED, _quadrature("ParallelNeuralIntegral", True)),
    ("NeuralIntegral", COMPILED, _quadrature("NeuralIntegral", False)),
    ("IntegralWithJacobian with a g_fx cotangent", COMPILED, _quadrature("IntegralWithJacobian", False)),
    ("MonotonicNN forward / backward", INDUCTOR, _monotonic(False)),
    ("MonotonicNN.inverse", COMPILED, _monotonic(True)),
    ("InverseNeuralIntegral, gradients to h and the parameters", COMPILED, _inverse_integral),
] + [(f"flow.invert {method}{', context' if cond else ' (raw_rows)'}", COMPILED, _invert(method, cond))
     for method in ("bracket", "newton", "jacobi") for cond in (False, True)] + _backward_plan_cases() + [
    ("forward plan: flow block", EAGER, _plan_block_case(False)), ("forward plan: ll block", EAGER, _plan_block_case(True)),
] + _forward_plan_cases() + _conditioner_cases() + [
    ("flow.invert newton, progressive conditioner", EAGER, _progressive_invert(False)),
    ("flow.invert newton, progressive conditioner, context", EAGER, _progressive_invert(True)),
    ("GraphedLL capture and two replays", EAGER, _graphed_ll),
]


def _flat(out):
    if out is None:
        return []
    if isinstance(out, torch.Tensor):
        return [out]
    return [t for o in out for t in _flat(o)]


def _have_triton():
    try:
        import triton  # noqa: F401
        return True
    except ImportError:
        return False


def run(out_path):
    import torch._dynamo
    import umnn_amd
    from umnn_amd import _lib
    dev = torch.device("cuda:0")
    lib = _lib.lib()
    records = []
    warnings.simplefilter("ignore")
    print("package:", os.path.dirname(umnn_amd.__file__), flush=True)
    for name, backends, make in CASES:
        for backend in backends:
            if backend == "inductor" and not _have_triton():
                continue
            torch._dynamo.reset()
            rec = {"case": name, "backend": backend, "tensors": [], "error": None}
            try:
                model, fn, tensors, after = make(dev)
                if backend != "eager":
                    fn = torch.compile(fn, backend=backend)
                torch.cuda.synchronize()
                n0, m0 = lib.umnn_launch_count(), lib.umnn_made_launch_count()
                out = fn(*tensors)
                outs = _flat(out)
                more = _flat(after(model, out, tensors)) if after is not None else []
                torch.cuda.synchronize()
                rec["tensors"] = [t.detach().cpu().clone() for t in outs + more]
                rec["launches"] = int(lib.umnn_launch_count() - n0)
                rec["path"], rec["backward_path"] = umnn_amd.path_taken(), umnn_amd.backward_path_taken()
                rec["kernel"] = lib.umnn_last_kernel_name().decode()
                rec["bwd_kernel"] = lib.umnn_last_kernel_name_of(_lib.PROF_BACKWARD).decode()
                rec["made_launches"], rec["made_kernel"] = int(lib.umnn_made_launch_count() - m0), lib.umnn_last_made_kernel_name().decode()
            except Exception as e:      # noqa: BLE001  (recorded: both checkouts must fail alike)
                rec["error"] = type(e).__name__
            records.append(rec)
            print(f"{name} [{backend}]: {len(rec['tensors'])} tensors, {rec.get('launches')} launches, {rec.get('path')} / "
                  f"{rec.get('backward_path')}, {rec.get('kernel')}, {rec.get('bwd_kernel')}, conditioner {rec.get('made_launches')} x {rec.get('made_kernel')}{', ' + rec['error'] if rec['error'] else ''}", flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    torch.save(records, out_path)


def compare(a_path, b_path, report=None):
    a, b = torch.load(a_path), torch.load(b_path)
    lines, tensors, bad, kernels = [], 0, 0, set()
    if [(r["case"], r["backend"]) for r in a] != [(r["case"], r["backend"]) for r in b]:
        lines.append("MISMATCH: the two files do not hold the same cases")
        bad += 1
    for ra, rb in zip(a, b):
        where = f"{ra['case']} [{ra['backend']}]"
        for key in ("error", "launches", "path", "backward_path", "kernel", "bwd_kernel", "made_launches", "made_kernel"):
            if ra.get(key) != rb.get(key):
                bad += 1
                lines.append(f"MISMATCH {where}: {key} {ra.get(key)!r} != {rb.get(key)!r}")
        if len(ra["tensors"]) != len(rb["tensors"]):
            bad += 1
            lines.append(f"MISMATCH {where}: {len(ra['tensors'])} tensors != {len(rb['tensors'])}")
        for i, (ta, tb) in enumerate(zip(ra["tensors"], rb["tensors"])):
            tensors += 1
            same = ta.shape == tb.shape and ta.dtype == tb.dtype and torch.equal(ta, tb)
            if not same and ta.shape == tb.shape and ta.dtype == tb.dtype:       # (torch.equal is False on NaN: compare the bits)
                same = torch.equal(ta.contiguous().view(torch.uint8), tb.contiguous().view(torch.uint8))
            if not same:
                bad += 1
                lines.append(f"MISMATCH {where}: tensor {i} {tuple(ta.shape)} {ta.dtype} vs {tuple(tb.shape)} {tb.dtype}")
        kernels.update(k for k in (ra.get("kernel"), ra.get("bwd_kernel"), ra.get("made_kernel")) if k)
        if ra["error"]:
            lines.append(f"note {where}: both raised {ra['error']}" if ra["error"] == rb["error"] else "")
    head = [f"cases x backends: {len(a)}", f"tensors compared: {tensors}", f"mismatches: {bad}", "kernel names seen:"]
    text = "\n".join(head + sorted("  " + k for k in kernels) + [l for l in lines if l]) + "\n"
    print(text, end="")
    if report:
        with open(report, "w") as f:
            f.write(text)
    return 1 if bad else 0


if __name__ == "__main__":
    if len(sys.argv) >= 3 and sys.argv[1] == "run":
        run(sys.argv[2])
    elif len(sys.argv) >= 4 and sys.argv[1] == "compare":
        sys.exit(compare(sys.argv[2], sys.argv[3], sys.argv[4] if len(sys.argv) > 4 else None))
    else:
        sys.exit(__doc__)
