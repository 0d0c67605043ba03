#!/usr/bin/env python
"""Times ``MonotonicNN.forward_curve`` against what a user can do without it.

Workload: ``MonotonicNN(3, [100, 100, 100], nb_steps=50, n_out=K)``, K in {2, 4, 16}, 8192 and 65 536 rows, under ``torch.no_grad()``.
Per (K, rows) these variants, all in one process, warmed up, then ``--reps`` rounds that alternate them, a pair of device events
around every call (milliseconds; median, min, max per variant as one JSON line each):

    forward_curve      the API: conditioner, node launch, cumulate launch, elementwise glue -> (t, y) on n + 1 abscissae per row
    cif                ``cumulative_incidence(curve=True)``: forward_curve with dy/dt, the integrand, one more cumulate launch
    nodes              the node launch alone (``integral.hip_forward_multi_nodes``)
    cumulate           the cumulate launch alone (``integral.hip_cumulate``)
    repeat (a)         one ``forward`` on the B (n + 1) rows (t_i, h repeated): the same curve, the best a user can do today
    repeat_kernel      its quadrature launch alone (``integral.hip_forward_multi`` on B (n + 1) rows)
    forward (b)        one ``forward`` of the B rows -- the end point only: the floor
    forward_kernel     its quadrature launch alone

A ``summary`` line per cell gives forward_curve / repeat, nodes / forward_kernel, cumulate / nodes and the largest difference between
the curve and the repeated forward (``rel_err`` = max |a - b| / max(|b|, 1): two quadratures of the same function, so this is
quadrature error, not arithmetic).  A cell whose tensors would not fit the free device memory is skipped, and a ``skipped`` line
says so.  Kernel times are a separate run:  rocprofv3 --kernel-trace --stats -d DIR -- python tools/curve_bench.py --reps 2 --only-k 4

    python tools/curve_bench.py [--reps 10] [--warmup 2] [--rows 8192,65536] [--nb-steps 50] [--only-k 2,4,16] [--out FILE.jsonl]

``--grad`` times TRAINING through the curves instead: forward plus backward (gradients in x, h and every parameter) of

    curve_hip / curve_aten     ``forward_curve(with_derivative=True, backward=...)`` under the loss sum(y G1) + sum(dy/dt G2)
    cif_hip / cif_aten         ``cumulative_incidence(curve=True, backward=...)`` under sum(CIF G1)
    forward                    the plain ``forward`` of the B end points and its backward, for scale

same net, rows, process and alternation.  An ATen variant whose autograd graph (B (n + 1) rows through every layer, kept) would not
fit the free device memory is skipped and reported; the ``summary`` line gives aten / hip and the largest ``scaled_err`` between the
two paths' gradients, per-row ones (dx, dh) and parameters apart: the same discretised gradient, so this is rounding -- and, on
random rows of an untrained ReLU net, the rows where a pre-activation sits within rounding of its kink and the two paths take
different sides (the tests hold cases of known kink margin to 1e-5).
"""
import argparse
import json
import os
import statistics
import sys


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--rows", default="8192,65536")
    ap.add_argument("--nb-steps", type=int, default=50)
    ap.add_argument("--only-k", default="2,4,16")
    ap.add_argument("--out", default=None)
    ap.add_argument("--grad", action="store_true")
    args = ap.parse_args()
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import torch
    import umnn_amd
    from umnn_amd import integral as I
    from umnn_amd.nets import mlp_spec

    assert torch.cuda.is_available(), "curve_bench needs a GPU"
    dev = torch.device("cuda:0")
    lines = []

    def emit(rec):
        line = json.dumps(rec)
        print(line, flush=True)
        lines.append(line)

    def timed(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        return a.elapsed_time(b)

    if args.grad:
        grad_cells(args, torch, umnn_amd, dev, emit, timed)
        if args.out:
            with open(args.out, "w") as f:
                f.write("\n".join(lines) + "\n")
        return

    n = args.nb_steps
    for K in [int(k) for k in args.only_k.split(",") if k]:
        for B in [int(r) for r in args.rows.split(",") if r]:
            # the largest tensors alive at once: f_nodes, C, their flipped / scaled copies and the repeated forward's rows
            need = 4 * B * (n + 1) * (8 * K + 8)
            free = torch.cuda.mem_get_info(dev)[0]
            if need > 0.8 * free:
                emit(dict(kind="skipped", K=K, rows=B, need_bytes=need, free_bytes=free))
                continue
            torch.manual_seed(K)
            m = umnn_amd.MonotonicNN(3, [100, 100, 100], nb_steps=n, n_out=K).to(dev)
            spec = mlp_spec(m.integrand)
            gen = torch.Generator(device="cpu").manual_seed(1000 + K)
            x = (torch.rand(B, 1, generator=gen) * 4 + 0.1).to(dev)
            h = torch.randn(B, 2, generator=gen).to(dev)
            with torch.no_grad():
                t, y = m.forward_curve(x, h)
                f_nodes = I.hip_forward_multi_nodes(spec, None, x, h, n)[1]
                tr = t.reshape(-1, 1).contiguous()
                hr = h.repeat_interleave(n + 1, 0).contiguous()
                y_rep = m(tr, hr).view(B, n + 1, K)
                err = float(((y - y_rep).abs() / y_rep.abs().clamp(min=1.)).max())
                end = float(((y[:, -1] - m(x, h)).abs() / m(x, h).abs().clamp(min=1.)).max())
            del y_rep
            variants = {
                "forward_curve": lambda: m.forward_curve(x, h),
                "cif": lambda: m.cumulative_incidence(x, h, curve=True),
                "nodes": lambda: I.hip_forward_multi_nodes(spec, None, x, h, n),
                "cumulate": lambda: I.hip_cumulate(f_nodes, None, x, n),
                "repeat": lambda: m(tr, hr),
                "repeat_kernel": lambda: I.hip_forward_multi(spec, None, tr, hr, n),
                "forward": lambda: m(x, h),
                "forward_kernel": lambda: I.hip_forward_multi(spec, None, x, h, n),
            }
            times = {k: [] for k in variants}
            with torch.no_grad():
                for _ in range(args.warmup):
                    for fn in variants.values():
                        fn()
                torch.cuda.synchronize()
                for _ in range(args.reps):
                    for name, fn in variants.items():
                        times[name].append(timed(fn))
            med = {k: statistics.median(v) for k, v in times.items()}
            for name, v in times.items():
                emit(dict(kind="time", K=K, rows=B, nb_steps=n, variant=name, median_ms=med[name], min_ms=min(v), max_ms=max(v), reps=len(v)))
            emit(dict(kind="summary", K=K, rows=B, nb_steps=n, curve_over_repeat=med["forward_curve"] / med["repeat"],
                      nodes_over_forward_kernel=med["nodes"] / med["forward_kernel"], cumulate_over_nodes=med["cumulate"] / med["nodes"],
                      kernels_over_repeat_kernel=(med["nodes"] + med["cumulate"]) / med["repeat_kernel"],
                      curve_vs_repeat_rel_err=err, end_point_vs_forward_rel_err=end))
            del f_nodes, tr, hr, t, y
            torch.cuda.empty_cache()
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


def grad_cells(args, torch, umnn_amd, dev, emit, timed):
    import warnings
    warnings.simplefilter("ignore")                 # (the one-time notice of the ATen route)
    n = args.nb_steps
    for K in [int(k) for k in args.only_k.split(",") if k]:
        for B in [int(r) for r in args.rows.split(",") if r]:
            torch.manual_seed(K)
            m = umnn_amd.MonotonicNN(3, [100, 100, 100], nb_steps=n, n_out=K).to(dev)
            params = list(m.parameters())
            gen = torch.Generator(device="cpu").manual_seed(1000 + K)
            x = (torch.rand(B, 1, generator=gen) * 4 + 0.1).to(dev)
            h = torch.randn(B, 2, generator=gen).to(dev)
            G1 = torch.randn(B, n + 1, K, generator=gen).to(dev)
            G2 = torch.randn(B, n + 1, K, generator=gen).to(dev)
            Gy = torch.randn(B, K, generator=gen).to(dev)

            def grads(loss_fn):
                xr, hr = x.clone().requires_grad_(), h.clone().requires_grad_()
                return torch.autograd.grad(loss_fn(xr, hr), [xr, hr] + params)

            def curve(backward):
                def loss(xr, hr):
                    _, y, dy = m.forward_curve(xr, hr, with_derivative=True, backward=backward)
                    return (y * G1).sum() + (dy * G2).sum()
                return lambda: grads(loss)

            def cif(backward):
                return lambda: grads(lambda xr, hr: (m.cumulative_incidence(xr, hr, curve=True, backward=backward)[1] * G1).sum())

            variants = {"curve_hip": curve("hip"), "cif_hip": cif("hip"), "forward": lambda: grads(lambda xr, hr: (m(xr, hr) * Gy).sum())}
            # ATen under autograd keeps, per hidden layer, the pre-activation, the activation and its mask for B (n + 1) rows, and about
            # a dozen [B, n + 1, K] tensors of the curve's own glue; the backward holds as much again in cotangents
            need = 2 * 4 * B * (n + 1) * (3 * 3 * 100 + 12 * K)
            free = torch.cuda.mem_get_info(dev)[0]
            if need > 0.8 * free:
                emit(dict(kind="skipped", K=K, rows=B, variants=["curve_aten", "cif_aten"], need_bytes=need, free_bytes=free))
            else:
                variants.update(curve_aten=curve("aten"), cif_aten=cif("aten"))
            err = {}
            if "curve_aten" in variants:
                for tag in ("curve", "cif"):
                    a, b = variants[tag + "_hip"](), variants[tag + "_aten"]()
                    each = [float((u - v).abs().max() / v.abs().max().clamp(min=1e-30)) for u, v in zip(a, b)]
                    err[tag], err[tag + "_params"] = max(each[:2]), max(each[2:])        # per row (dx, dh); summed over the rows
                    del a, b
            times = {k: [] for k in variants}
            for _ in range(args.warmup):
                for fn in variants.values():
                    fn()
            torch.cuda.synchronize()
            for _ in range(args.reps):
                for name, fn in variants.items():
                    times[name].append(timed(fn))
            med = {k: statistics.median(v) for k, v in times.items()}
            for name, v in times.items():
                emit(dict(kind="time", K=K, rows=B, nb_steps=n, variant=name, median_ms=med[name], min_ms=min(v), max_ms=max(v), reps=len(v)))
            emit(dict(kind="summary", K=K, rows=B, nb_steps=n,
                      curve_aten_over_hip=med["curve_aten"] / med["curve_hip"] if "curve_aten" in med else None,
                      cif_aten_over_hip=med["cif_aten"] / med["cif_hip"] if "cif_aten" in med else None,
                      curve_hip_over_forward=med["curve_hip"] / med["forward"],
                      curve_rows_hip_vs_aten_scaled_err=err.get("curve"), curve_params_hip_vs_aten_scaled_err=err.get("curve_params"),
                      cif_rows_hip_vs_aten_scaled_err=err.get("cif"), cif_params_hip_vs_aten_scaled_err=err.get("cif_params")))
            del G1, G2
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
