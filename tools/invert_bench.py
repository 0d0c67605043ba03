#!/usr/bin/env python
"""Times the sampling direction: one block's ``invert(iter=10)`` (the bracket search) against ``invert(method="newton")`` and
``invert(method="jacobi")`` at the C3 block (8192 x 63, 31-50^4-1, n = 100) and the MNIST-shaped block (100 x 784, 31-100-50^4-1,
n = 100) -- each with default-initialised weights and again with the MADE weights times 3 (cases ``c3_made3`` / ``mnist_made3``:
stronger coupling between the dimensions, more Jacobi sweeps) --, and ``MonotonicNN.inverse`` at 65 536 x 1 with the 3-100^3-1 net
of the g5 fixtures.  The jacobi rows carry the sweep count and the largest evaluation count of every sweep.

    python tools/invert_bench.py [--repeats 5] [--warmup 1] [--root TREE] [--out FILE.json] [--only c3,mnist,c3_made3,mnist_made3,monotonic,toy]
                                 [--methods bracket,newton,newton_progressive,jacobi] [--conditioner full|progressive]

Device-synchronised wall time of whole calls (conditioner passes included), ``--warmup`` untimed calls of every method first, then
``--repeats`` rounds that alternate the methods, so drift hits both alike; every figure comes with its min / max / standard
deviation.  ``--grad`` times the gradient through a sample instead (the same block shapes): ``rsample`` and the backward of
``x.square().sum()`` with the default stop rule (row ``rsample_backward``: the sweep counts of that backward), the same backward at
two fixed sweep counts (``adj_tol=0``, ``max_adj_sweeps`` 2 and 6: their difference over 4 is the time of ONE sweep, printed as
``ms_per_sweep``), and one training backward of the block (``-compute_ll(x).mean()``, parameters and x requiring grad) to hold a sweep
against -- the one row a tree without ``inverse`` (``--root``) also gives; ``--methods`` selects rows by name there (a kernel trace
of the sweeps alone: ``--grad --methods rsample_backward_6_sweeps --repeats 1 --warmup 0``: seven launches of the main backward
kernel, one parameter reduction).  ``--root`` imports the package from another checkout (a tree without the Newton method -- the parent of this change --
times the bracket search only), which is how the same-box comparison against an older build is taken.  ``--graph`` times eager
``invert`` against ``umnn_amd.GraphedSampler`` replays (rows ``newton`` / ``newton_graph`` and ``jacobi`` / ``jacobi_graph``, alternating
in every round; given noise copied into the static buffer, so both sides solve the same z) at the C3 block, the MNIST-shaped block and
the 2-D toy flow of bench.py (case ``toy``: 4096 x 2, one block); the jacobi pair runs ``sweep_tol=0`` with ``max_sweeps`` set to the
sweep count eager jacobi needed with its default stop rule (row field ``sweeps``), ``capture_ms`` is the one-time cost of building the
sampler (warm-up + capture).  Per-launch kernel time is
a separate run:  rocprofv3 --kernel-trace --stats -d DIR -- python tools/invert_bench.py --repeats 1 --only c3
Row ``newton_progressive`` is ``invert(method="newton", conditioner="progressive")`` (under ``--graph`` also ``newton_progressive_graph``,
its ``GraphedSampler`` replay); ``--conditioner`` sets the conditioner of the ``bracket`` and ``newton`` rows themselves (default "full").
Every row carries ``made_launches``, the conditioner-kernel launches of its last call (progressive: d per block).  A tree without the
option (``--root``) gives the other rows only.
``--log-prob`` times the sample WITH its log-density: per method (``newton``, ``newton_progressive``, ``jacobi``) the rows ``<method>_sample``
(``flow.sample(n)``), ``<method>_sample_and_log_prob`` (``flow.sample_and_log_prob(n)``: the density from the solves that drew the sample)
and ``<method>_sample_then_log_prob`` (``sample`` followed by ``log_prob(x)``: a second conditioner and quadrature pass), alternating in
every round on the same seeded noise, at the C3 block (case ``c3``), the five-block C3 flow (``c3_flow``) and the MNIST-shaped block
(``mnist``); every row carries ``max_abs_dev_log_prob``, its density against ``log_prob(x)`` of its own x.
"""
import argparse
import inspect
import json
import os
import statistics
import sys
import time


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    ap.add_argument("--out", default=None)
    ap.add_argument("--only", default=ap_default_only)
    ap.add_argument("--methods", default=ap_default_methods)
    ap.add_argument("--label", default="")
    ap.add_argument("--conditioner", default="full", choices=["full", "progressive"], help="conditioner of the bracket and newton rows")
    ap.add_argument("--adj-tol", type=float, default=None, help="--grad: adj_tol of the rsample_backward row (default: the method's own)")
    ap.add_argument("--grad", action="store_true", help="time rsample + backward and the adjoint sweeps instead of the solves")
    ap.add_argument("--graph", action="store_true", help="time eager invert against GraphedSampler replays (newton and fixed-sweep jacobi)")
    ap.add_argument("--log-prob", action="store_true", help="time sample, sample_and_log_prob and sample + log_prob (newton, both conditioners; jacobi)")
    args = ap.parse_args()
    sys.path.insert(0, os.path.abspath(args.root))
    import torch
    import umnn_amd
    from umnn_amd import _lib

    dev = torch.device("cuda:0")
    has_newton = "method" in inspect.signature(umnn_amd.UMNNMAF.invert).parameters
    has_jacobi = "sweep_tol" in inspect.signature(umnn_amd.UMNNMAF.invert).parameters
    has_progressive = "conditioner" in inspect.signature(umnn_amd.UMNNMAF.invert).parameters
    if args.conditioner != "full" and not has_progressive:
        raise SystemExit("--conditioner: this tree's invert has no such option")
    cond = dict(conditioner=args.conditioner) if args.conditioner != "full" else {}
    only = set(args.only.split(","))
    methods = set(args.methods.split(","))

    def sync_time(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, out

    def measure(case, fns, extra):
        """fns: {method: callable}; alternates them every round."""
        for _ in range(args.warmup):
            for fn in fns.values():
                sync_time(fn)
        ms = {k: [] for k in fns}
        launches, made_launches, kernels, outs = {}, {}, {}, {}
        for _ in range(args.repeats):
            for k, fn in fns.items():
                n0, m0 = _lib.lib().umnn_launch_count(), _lib.lib().umnn_made_launch_count()
                t, outs[k] = sync_time(fn)
                ms[k].append(t)
                launches[k] = _lib.lib().umnn_launch_count() - n0
                made_launches[k] = _lib.lib().umnn_made_launch_count() - m0
                kernels[k] = _lib.lib().umnn_last_kernel_name().decode()
        rows = []
        for k, v in ms.items():
            rows.append(dict(case=case, method=k, label=args.label, mean_ms=statistics.mean(v), min_ms=min(v), max_ms=max(v),
                             std_ms=statistics.pstdev(v), repeats=len(v), launches=launches[k], made_launches=made_launches[k],
                             kernel=kernels[k], **extra(k, outs)))
            print(json.dumps(rows[-1]), flush=True)
        return rows

    results = []
    shapes = {"c3": dict(d=63, hd=[50] * 4, he=[512, 512], E=30, n=100, B=8192),
              "mnist": dict(d=784, hd=[100, 50, 50, 50, 50], he=[1024] * 3, E=30, n=100, B=100)}
    if args.grad:
        results += grad_mode(args, umnn_amd, torch, dev, shapes, only, measure)
        only = set()
    if args.graph:
        results += graph_mode(args, umnn_amd, torch, dev, shapes, only if args.only != ap_default_only else {"c3", "mnist", "toy"},
                              methods, measure, sync_time, has_progressive, cond)
        only = set()
    if args.log_prob:
        results += log_prob_mode(args, umnn_amd, torch, dev, shapes, only if args.only != ap_default_only else {"c3", "c3_flow", "mnist"},
                                 methods, measure)
        only = set()
    with torch.no_grad():
        for case, c in [(name + tag, dict(c, made_gain=gain)) for name, c in shapes.items() for tag, gain in (("", 1.), ("_made3", 3.))]:
            if case not in only:
                continue
            torch.manual_seed(0)
            flow = umnn_amd.UMNNMAFFlow(nb_flow=1, nb_in=c["d"], hidden_derivative=c["hd"], hidden_embedding=c["he"],
                                        embedding_s=c["E"], nb_steps=c["n"], solver="CCParallel").to(dev).eval()
            blk = flow.nets[0]
            if c["made_gain"] != 1.:
                for mod in blk.net.made.net:
                    if hasattr(mod, "weight"):
                        mod.weight.mul_(c["made_gain"])
                umnn_amd.invalidate_caches(flow)
            x = torch.randn(c["B"], c["d"], device=dev)
            z = blk(x)
            fns, state = {}, {}
            if "bracket" in methods:
                fns["bracket"] = lambda: blk.invert(z, iter=10, **cond)
            if has_newton and "newton" in methods:
                fns["newton"] = lambda: blk.invert(z, method="newton", **cond)
            if has_progressive and "newton_progressive" in methods:
                fns["newton_progressive"] = lambda: blk.invert(z, method="newton", conditioner="progressive")
            if has_jacobi and "jacobi" in methods:
                def jacobi():
                    xi, state["info"] = blk.invert(z, method="jacobi", return_info=True)
                    return xi
                fns["jacobi"] = jacobi

            def extra(k, outs, x=x, state=state):
                out = dict(max_abs_err_x=float((outs[k] - x).abs().max()))
                if k == "jacobi":
                    info = state["info"]
                    out.update(sweeps=info["sweeps"], converged=info["converged"], max_evals_per_sweep=info["max_evals"])
                return out
            results += measure(case, fns, extra)
        if "monotonic" in only and hasattr(umnn_amd.MonotonicNN, "inverse"):
            torch.manual_seed(0)
            m = umnn_amd.MonotonicNN(3, [100, 100, 100], nb_steps=50).to(dev)
            B = 65536
            x, h = torch.randn(B, 1, device=dev) * 2, torch.randn(B, 2, device=dev)
            y = m(x, h)
            state = {}

            def inverse():
                xi, _, status = m.inverse(y, h, return_info=True)
                state["evals"] = status
                return xi

            def extra(k, outs):
                if k != "inverse":
                    return {}
                ev = (state["evals"] & umnn_amd.SOLVE_EVALS_MASK).float()
                return dict(max_abs_err_x=float((outs[k] - x).abs().max()), mean_evals=float(ev.mean()), max_evals=int(ev.max()))
            results += measure("monotonic_65536", {"forward": lambda: m(x, h), "inverse": inverse}, extra)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(dict(device=torch.cuda.get_device_name(0), precision=umnn_amd.get_forward_precision(), label=args.label,
                           has_newton=has_newton, results=results), f, indent=1)


ap_default_methods = "bracket,newton,newton_progressive,jacobi"
ap_default_only = "c3,mnist,c3_made3,mnist_made3,monotonic"


def graph_mode(args, umnn_amd, torch, dev, shapes, only, methods, measure, sync_time, has_progressive=False, cond={}):
    """The ``--graph`` rows: eager ``invert`` and the replay of a ``GraphedSampler`` on the same z, per method."""
    results = []
    shapes = dict(shapes, toy=dict(d=2, hd=[100] * 4, he=[100] * 4, E=10, n=50, B=4096))
    with torch.no_grad():
        for case, c in shapes.items():
            if case not in only:
                continue
            torch.manual_seed(0)
            flow = umnn_amd.UMNNMAFFlow(nb_flow=1, nb_in=c["d"], hidden_derivative=c["hd"], hidden_embedding=c["he"],
                                        embedding_s=c["E"], nb_steps=c["n"], solver="CCParallel").to(dev).eval()
            x = torch.randn(c["B"], c["d"], device=dev)
            z = flow(x)
            fns, meta = {}, {}
            if "newton" in methods:
                ms, sampler = sync_time(lambda: umnn_amd.GraphedSampler(flow, c["B"], method="newton", **cond))
                meta["newton_graph"] = dict(capture_ms=ms)
                fns["newton"] = lambda: flow.invert(z, method="newton", **cond)
                fns["newton_graph"] = lambda sampler=sampler: sampler(z=z)
            if has_progressive and "newton_progressive" in methods:
                ms, psampler = sync_time(lambda: umnn_amd.GraphedSampler(flow, c["B"], method="newton", conditioner="progressive"))
                meta["newton_progressive_graph"] = dict(capture_ms=ms)
                fns["newton_progressive"] = lambda: flow.invert(z, method="newton", conditioner="progressive")
                fns["newton_progressive_graph"] = lambda psampler=psampler: psampler(z=z)
            if "jacobi" in methods:
                _, info = flow.invert(z, method="jacobi", return_info=True)
                K = max(info["sweeps"])
                ms, jsampler = sync_time(lambda: umnn_amd.GraphedSampler(flow, c["B"], method="jacobi", sweep_tol=0, max_sweeps=K))
                meta["jacobi"] = dict(sweeps=K)
                meta["jacobi_graph"] = dict(sweeps=K, capture_ms=ms)
                fns["jacobi"] = lambda K=K: flow.invert(z, method="jacobi", sweep_tol=0, max_sweeps=K)
                fns["jacobi_graph"] = lambda jsampler=jsampler: jsampler(z=z)

            def extra(k, outs, x=x, meta=meta):
                out = dict(max_abs_err_x=float((outs[k] - x).abs().max()), **meta.get(k, {}))
                if k == "jacobi_graph":
                    out["last_move"] = float(jsampler.last_move)
                return out
            results += measure(case, fns, extra)
            del flow, fns
            torch.cuda.empty_cache()
    return results


def log_prob_mode(args, umnn_amd, torch, dev, shapes, only, methods, measure):
    """The ``--log-prob`` rows: ``sample``, ``sample_and_log_prob`` and ``sample`` + ``log_prob`` per method, on the same seeded noise."""
    results = []
    cases = {"c3": dict(shapes["c3"], nb_flow=1), "c3_flow": dict(shapes["c3"], nb_flow=5), "mnist": dict(shapes["mnist"], nb_flow=1)}
    solve = {"newton": dict(method="newton"), "newton_progressive": dict(method="newton", conditioner="progressive"),
             "jacobi": dict(method="jacobi")}
    with torch.no_grad():
        for case, c in cases.items():
            if case not in only:
                continue
            torch.manual_seed(0)
            flow = umnn_amd.UMNNMAFFlow(nb_flow=c["nb_flow"], nb_in=c["d"], hidden_derivative=c["hd"], hidden_embedding=c["he"],
                                        embedding_s=c["E"], nb_steps=c["n"], solver="CCParallel").to(dev).eval()
            B = c["B"]

            def gen():
                return torch.Generator(device=dev).manual_seed(1)

            fns = {}
            for m, o in solve.items():
                if m not in methods:
                    continue
                fns[m + "_sample"] = lambda o=o: (flow.sample(B, generator=gen(), **o), None)
                fns[m + "_sample_and_log_prob"] = lambda o=o: flow.sample_and_log_prob(B, generator=gen(), **o)

                def two_calls(o=o):
                    x = flow.sample(B, generator=gen(), **o)
                    return x, flow.log_prob(x)
                fns[m + "_sample_then_log_prob"] = two_calls

            def extra(k, outs):
                x, lp = outs[k]
                out = dict(nb_flow=c["nb_flow"], B=B, d=c["d"])
                if lp is not None:
                    ref = flow.log_prob(x)
                    out["max_abs_dev_log_prob"] = float((lp - ref).abs().max())
                    out["max_rel_dev_log_prob"] = float(((lp - ref).abs() / ref.abs().clamp(min=1.)).max())
                return out
            results += measure(case, fns, extra)
            del flow, fns
            torch.cuda.empty_cache()
    return results


def grad_mode(args, umnn_amd, torch, dev, shapes, only, measure):
    """The ``--grad`` rows of every block shape in ``only``."""
    results = []
    has_inverse = hasattr(umnn_amd.UMNNMAFFlow, "rsample")
    for case, c in [(name + tag, dict(c, made_gain=gain)) for name, c in shapes.items() for tag, gain in (("", 1.), ("_made3", 3.))]:
        if case not in only:
            continue
        torch.manual_seed(0)
        flow = umnn_amd.UMNNMAFFlow(nb_flow=1, nb_in=c["d"], hidden_derivative=c["hd"], hidden_embedding=c["he"],
                                    embedding_s=c["E"], nb_steps=c["n"], solver="CCParallel").to(dev)
        if c["made_gain"] != 1.:
            with torch.no_grad():
                for mod in flow.nets[0].net.made.net:
                    if hasattr(mod, "weight"):
                        mod.weight.mul_(c["made_gain"])
            umnn_amd.invalidate_caches(flow)
        params = [p for p in flow.parameters() if p.requires_grad]
        state = {}

        def timed_backward(make_loss):
            """Forward untimed, then the backward alone between two device synchronisations (the row's ``backward_ms``)."""
            loss = make_loss()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            grads = torch.autograd.grad(loss, params, allow_unused=True)
            torch.cuda.synchronize()
            state.setdefault("bwd", []).append((time.perf_counter() - t0) * 1e3)
            return grads

        x_train = torch.randn(c["B"], c["d"], device=dev, requires_grad=True)

        def train_backward():
            return timed_backward(lambda: -flow.compute_ll(x_train)[0].mean())

        def rsample_backward(**kw):
            def make_loss():
                x, state["info"] = flow.rsample(c["B"], generator=torch.Generator(device=dev).manual_seed(1), return_info=True, **kw)
                return x.square().sum()
            return timed_backward(make_loss)

        fns = {"train_backward": train_backward}
        if has_inverse:
            fns["rsample_backward"] = (lambda: rsample_backward(adj_tol=args.adj_tol)) if args.adj_tol is not None else rsample_backward
            fns["rsample_backward_2_sweeps"] = lambda: rsample_backward(adj_tol=0., max_adj_sweeps=2)
            fns["rsample_backward_6_sweeps"] = lambda: rsample_backward(adj_tol=0., max_adj_sweeps=6)
        if args.methods != ap_default_methods:        # (a kernel trace of one row: --methods rsample_backward_6_sweeps --repeats 1 --warmup 0)
            fns = {k: fn for k, fn in fns.items() if k in args.methods.split(",")}
        bwd = {}

        def extra(k, outs):
            # (measure() calls this once per method after the rounds, in order: hand every method its own backward timings)
            if not bwd:
                per, n = state["bwd"][args.warmup * len(fns):], len(fns)
                for i, name in enumerate(fns):
                    bwd[name] = per[i::n]
            v = bwd[k]
            out = dict(backward_ms=statistics.mean(v), backward_min_ms=min(v), backward_max_ms=max(v), backward_std_ms=statistics.pstdev(v))
            if k == "rsample_backward":
                out.update(adjoint=state_default.get("adjoint"), adj_tol=args.adj_tol)
            return out

        state_default = {}
        if "rsample_backward" in fns:                 # the default stop rule's sweep counts (one untimed call)
            x, info = flow.rsample(c["B"], generator=torch.Generator(device=dev).manual_seed(1), return_info=True,
                                   **({} if args.adj_tol is None else {"adj_tol": args.adj_tol}))
            torch.autograd.grad(x.square().sum(), params, allow_unused=True)
            state_default["adjoint"] = info["adjoint"]
        rows = measure(case, fns, extra)
        if "rsample_backward_2_sweeps" in fns and "rsample_backward_6_sweeps" in fns and "train_backward" in fns:
            per_sweep = (bwd["rsample_backward_6_sweeps"][i] - bwd["rsample_backward_2_sweeps"][i] for i in range(args.repeats))
            per_sweep = [v / 4. for v in per_sweep]
            row = dict(case=case, method="ms_per_sweep", label=args.label, mean_ms=statistics.mean(per_sweep), min_ms=min(per_sweep),
                       max_ms=max(per_sweep), std_ms=statistics.pstdev(per_sweep), repeats=len(per_sweep),
                       train_backward_ms=statistics.mean(bwd["train_backward"]),
                       sweep_over_train_backward=statistics.mean(per_sweep) / statistics.mean(bwd["train_backward"]))
            print(json.dumps(row), flush=True)
            rows.append(row)
        results += rows
        del flow, params, x_train
        torch.cuda.empty_cache()
    return results


if __name__ == "__main__":
    main()
