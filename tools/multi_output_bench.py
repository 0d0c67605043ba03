#!/usr/bin/env python
"""Times the multi-output quadrature against what the single-output kernels can do for the same function.

Workload: the integrand of ``MonotonicNN(3, [100, 100, 100], nb_steps=50, n_out=K)``, 65 536 rows, K in {2, 4, 16}.  Per K and per
direction (``fwd``: the forward; ``fwd_bwd``: forward + backward with every gradient -- d_x, d_h, d_theta) three variants:

    multi          one launch of the multi-output kernels (csrc/cc_multi.hip: exact fp32 whatever the precision options say)
    single_fp32    K launches of the single-output kernels on the same hidden layers, last layer sliced to row k, under
                   ``set_precision("fp32")``
    single_f16x3   the same K launches under the default precision (fp16 pieces forward, bf16 pieces backward)

    python tools/multi_output_bench.py [--reps 20] [--warmup 3] [--rows 65536] [--nb-steps 50] [--only-k 2,4,16] [--out FILE.jsonl]

Same process, every variant warmed up, then ``--reps`` rounds that alternate the three variants, one pair of device events around
every call; each JSON line carries the median, min, max and mean of its variant in milliseconds.  A ``gate`` line per (K, direction)
says whether multi is below the K fp32 launches (median against median) and gives multi / single ratios; a ``check`` line per K
compares each column against its single-output fp32 launch (``rel_err`` = max |a - b| / max(|b|, 1), bound 1e-5) and the summed
d_x / d_h of the K single backward launches against the multi backward.  Run the command twice to see the spread; kernel times are
a separate run:  rocprofv3 --kernel-trace --stats -d DIR -- python tools/multi_output_bench.py --reps 2 --warmup 1 --only-k 4

``--derivative`` times the differentiable pair (y, dy/dx) instead, forward + backward with d_x, d_h and d_theta, per K:

    pair           the multi-output forward and the backward with both cotangents (g, g_fx): umnn_cc_backward_multi_fx
    g_only         the same forward and the backward with g alone (the kernels without g_fx)
    two_eval       what one writes without the pair: g_only plus a second evaluation of f(x; h) in ATen, differentiated by autograd

and, through the C entries themselves with every buffer allocated once, ``abi_g_only`` twice in every round (``_a`` and ``_b``: their
medians differ by the run-to-run spread of this session) and -- with ``--root DIR``, a built checkout of another commit --
``abi_g_only_root`` on DIR/umnn_amd/libumnn_cc.so, alternating with them.  A ``derivative`` line per K gives pair / g_only against the
node count (n + 2) / (n + 1) of the first backward pass, pair / two_eval, the spread and root / new.

``--inverse-sum`` times the inverse of a weighted sum of the K curves, sum_k coef_k int_0^x f_k = t, per K at ``--rows`` rows and at 100:

    kernel         one launch of umnn_cc_solve_multi (``integral.hip_solve_multi``): the Newton iteration inside the kernel
    host_loop      ``integral.newton_solve_sum`` over ``hip_forward_multi``: one forward launch and a handful of elementwise launches
                   per iteration, with a sync for the stop test -- the only route without the solve kernel
    api            ``MonotonicNN.inverse_sum`` under no_grad: the conditioner, the elementwise glue and the kernel

Wall-clock milliseconds between two device synchronisations (the host loop's cost is largely host time), variants alternating
within a round.  A ``solve`` line per (K, rows) gives the launch counts of one call, the evaluations per row (mean, max) of both
routes, the largest |x_kernel - x_host| D in units of the stop bound tol max(1, |t|), and kernel / host_loop.
"""
import argparse
import json
import os
import statistics
import sys


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rows", type=int, default=65536)
    ap.add_argument("--nb-steps", type=int, default=50)
    ap.add_argument("--only-k", default="2,4,16")
    ap.add_argument("--out", default=None)
    ap.add_argument("--label", default="")
    ap.add_argument("--derivative", action="store_true")
    ap.add_argument("--root", default=None)
    ap.add_argument("--inverse-sum", action="store_true")
    args = ap.parse_args()
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import torch
    import umnn_amd
    from umnn_amd import _lib, integral as I
    from umnn_amd.nets import MlpSpec, TensorLinear, mlp_spec

    assert torch.cuda.is_available(), "multi_output_bench needs a GPU"
    dev = torch.device("cuda:0")
    default_precision = (umnn_amd.get_forward_precision(), umnn_amd.get_backward_precision())
    lines = []

    def emit(rec):
        rec = dict(rec, label=args.label) if args.label else rec
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

    def set_prec(fwd, bwd):
        umnn_amd.set_forward_precision(fwd)
        umnn_amd.set_backward_precision(bwd)

    n, B = args.nb_steps, args.rows
    need = (False, True, True, True)
    if args.derivative:
        derivative(args, emit, timed)
        args.only_k = ""
    if args.inverse_sum:
        inverse_sum(args, emit)
        args.only_k = ""
    for K in [int(k) for k in args.only_k.split(",") if k]:
        torch.manual_seed(K)
        m = umnn_amd.MonotonicNN(3, [100, 100, 100], nb_steps=n, n_out=K).to(dev)
        spec = mlp_spec(m.integrand)
        last = spec.linears[-1]
        rows = [MlpSpec(spec.linears[:-1] + [TensorLinear(last.weight[k:k + 1], last.bias[k:k + 1])], spec.hidden_act, spec.out_act)
                for k in range(K)]
        gen = torch.Generator(device="cpu").manual_seed(1000 + K)
        x = (torch.randn(B, 1, generator=gen) * 2).to(dev)
        h = torch.randn(B, 2, generator=gen).to(dev)
        g = torch.randn(B, K, generator=gen).to(dev)
        gk = [g[:, [k]].contiguous() for k in range(K)]

        def multi_fwd():
            return I.hip_forward_multi(spec, None, x, h, n)

        def multi_fwd_bwd():
            I.hip_forward_multi(spec, None, x, h, n)
            return I.hip_backward_multi(spec, None, x, h, g, n, need)

        def single_fwd():
            return [I.hip_forward(r, None, x, h, n) for r in rows]

        def single_fwd_bwd():
            out = []
            for k, r in enumerate(rows):
                I.hip_forward(r, None, x, h, n)
                out.append(I.hip_backward(r, None, x, h, gk[k], None, n, need))
            return out

        variants = {
            "multi": (default_precision, multi_fwd, multi_fwd_bwd),
            "single_fp32": (("fp32", "fp32"), single_fwd, single_fwd_bwd),
            "single_f16x3": (default_precision, single_fwd, single_fwd_bwd),
        }
        with torch.no_grad():
            # ---- results at the timed size
            set_prec("fp32", "fp32")
            cols = torch.cat([o[0] for o in single_fwd()], 1)
            sb = single_fwd_bwd()
            set_prec(*default_precision)
            F = multi_fwd()[0]
            kname = _lib.lib().umnn_last_kernel_name().decode()
            _, dx, dh, _ = multi_fwd_bwd()
            bname = _lib.lib().umnn_last_kernel_name_of(_lib.PROF_BACKWARD).decode()

            def rel(a, b):
                return float(((a - b).abs() / b.abs().clamp(min=1.)).max())

            def scaled(a, b):
                return float((a - b).abs().max() / b.abs().max().clamp(min=1e-30))

            emit({"kind": "check", "K": K, "rows": B, "nb_steps": n, "forward_kernel": kname, "backward_kernel": bname,
                  "columns_rel_err_vs_single_fp32": rel(F, cols), "bound": 1e-5,
                  "dx_scaled_err_vs_sum_of_single_fp32": scaled(dx, sum(o[1] for o in sb)),
                  "dh_scaled_err_vs_sum_of_single_fp32": scaled(dh, sum(o[2] for o in sb))})

            # ---- timings
            for di, direction in enumerate(("fwd", "fwd_bwd")):
                for name, (prec, *fns) in variants.items():
                    set_prec(*prec)
                    for _ in range(args.warmup):
                        fns[di]()
                torch.cuda.synchronize()
                times = {name: [] for name in variants}
                for _ in range(args.reps):
                    for name, (prec, *fns) in variants.items():
                        set_prec(*prec)
                        times[name].append(timed(fns[di]))
                set_prec(*default_precision)
                med = {}
                for name, ts in times.items():
                    med[name] = statistics.median(ts)
                    emit({"kind": "time", "K": K, "direction": direction, "variant": name, "rows": B, "nb_steps": n, "reps": len(ts),
                          "median_ms": med[name], "min_ms": min(ts), "max_ms": max(ts), "mean_ms": statistics.fmean(ts)})
                emit({"kind": "gate", "K": K, "direction": direction, "multi_below_K_single_fp32": med["multi"] < med["single_fp32"],
                      "multi_over_single_fp32": med["multi"] / med["single_fp32"],
                      "multi_over_single_f16x3": med["multi"] / med["single_f16x3"]})
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as f:
            f.write("\n".join(lines) + "\n")


def derivative(args, emit, timed):
    import ctypes
    import torch
    import umnn_amd
    from umnn_amd import _lib, integral as I
    from umnn_amd._common import _ptr, _stream
    from umnn_amd.nets import mlp_spec
    from umnn_amd.quadrature import device_tables

    dev = torch.device("cuda:0")
    n, B = args.nb_steps, args.rows
    need = (False, True, True, True)
    root = ctypes.CDLL(os.path.join(os.path.abspath(args.root), "umnn_amd", "libumnn_cc.so")) if args.root else None

    for K in [int(k) for k in args.only_k.split(",")]:
        torch.manual_seed(K)
        m = umnn_amd.MonotonicNN(3, [100, 100, 100], nb_steps=n, n_out=K).to(dev)
        spec = mlp_spec(m.integrand)
        gen = torch.Generator(device="cpu").manual_seed(1000 + K)
        x = (torch.randn(B, 1, generator=gen) * 2).to(dev)
        h = torch.randn(B, 2, generator=gen).to(dev)
        g = torch.randn(B, K, generator=gen).to(dev)
        gfx = torch.randn(B, K, generator=gen).to(dev)
        params = list(m.integrand.parameters())

        def g_only():
            I.hip_forward_multi(spec, None, x, h, n)
            return I.hip_backward_multi(spec, None, x, h, g, n, need)

        def pair():
            I.hip_forward_multi(spec, None, x, h, n)
            return I.hip_backward_multi(spec, None, x, h, g, n, need, g_fx=gfx)

        def two_eval():
            out = g_only()
            with torch.enable_grad():
                xr, hr = x.detach().requires_grad_(), h.detach().requires_grad_()
                return out, torch.autograd.grad((m.integrand(xr, hr) * gfx).sum(), [xr, hr] + params)

        def abi(handle):
            for nm in ("umnn_cc_forward_multi", "umnn_cc_backward_multi", "umnn_cc_backward_multi_workspace_bytes"):
                fn = getattr(handle, nm)
                fn.restype, fn.argtypes = _lib.SIGNATURES[nm]
            desc, keep = I._desc(spec)
            w, s = device_tables(n, dev)
            E = h.shape[1]
            F, fx, dx, dh = (torch.empty(B, c, device=dev) for c in (K, K, 1, E))
            dth = torch.empty(sum(p.numel() for p in params), device=dev)
            nbytes = handle.umnn_cc_backward_multi_workspace_bytes(ctypes.byref(desc), B, 1, E)
            ws = torch.empty(nbytes, device=dev, dtype=torch.uint8)
            held = (keep, w, s, F, fx, dx, dh, dth, ws)

            def run(held=held):
                st = _stream(dev)
                rc = handle.umnn_cc_forward_multi(ctypes.byref(desc), None, _ptr(x), _ptr(h), _ptr(w), _ptr(s), n, B, 1, E, 0, _ptr(F), _ptr(fx), None, st)
                rc |= handle.umnn_cc_backward_multi(ctypes.byref(desc), None, _ptr(x), _ptr(h), _ptr(g), _ptr(w), _ptr(s), n, B, 1, E, 0,
                                                    None, _ptr(dx), _ptr(dh), _ptr(dth), _ptr(ws), nbytes, st)
                assert rc == 0
                return dx, dh, dth
            return run

        new_abi = abi(ctypes.CDLL(_lib.LIB_PATH))
        variants = {"pair": pair, "g_only": g_only, "two_eval": two_eval, "abi_g_only_a": new_abi}
        if root is not None:
            variants["abi_g_only_root"] = abi(root)
        variants["abi_g_only_b"] = new_abi
        with torch.no_grad():
            if root is not None:
                a, b = [t.clone() for t in new_abi()], variants["abi_g_only_root"]()
                emit({"kind": "root_check", "K": K, "bit_equal_dx_dh_dtheta": [bool(torch.equal(u, v)) for u, v in zip(a, b)]})
            for fn in variants.values():
                for _ in range(args.warmup):
                    fn()
            torch.cuda.synchronize()
            times = {name: [] for name in variants}
            for _ in range(args.reps):
                for name, fn in variants.items():
                    times[name].append(timed(fn))
        med = {}
        for name, ts in times.items():
            med[name] = statistics.median(ts)
            emit({"kind": "time", "K": K, "direction": "fwd_bwd", "variant": name, "rows": B, "nb_steps": n, "reps": len(ts),
                  "median_ms": med[name], "min_ms": min(ts), "max_ms": max(ts), "mean_ms": statistics.fmean(ts)})
        new = 0.5 * (med["abi_g_only_a"] + med["abi_g_only_b"])
        emit({"kind": "derivative", "K": K, "pair_over_g_only": med["pair"] / med["g_only"], "node_count_of_the_first_pass": (n + 2) / (n + 1),
              "pair_over_two_eval": med["pair"] / med["two_eval"],
              "spread": abs(med["abi_g_only_a"] - med["abi_g_only_b"]) / new,
              "root_over_new": med["abi_g_only_root"] / new if root is not None else None})


def inverse_sum(args, emit):
    import time
    import torch
    import umnn_amd
    from umnn_amd import _lib, integral as I
    from umnn_amd.nets import mlp_spec

    dev = torch.device("cuda:0")
    n, tol, lo, hi, max_iter = args.nb_steps, 1e-6, -50., 50., 64
    launches = _lib.lib().umnn_launch_count

    def wall(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3

    for K in [int(k) for k in args.only_k.split(",")]:
        for B in (args.rows, 100):
            torch.manual_seed(K)
            m = umnn_amd.MonotonicNN(3, [100, 100, 100], nb_steps=n, n_out=K).to(dev)
            spec = mlp_spec(m.integrand)
            gen = torch.Generator(device="cpu").manual_seed(2000 + K)
            x = (torch.randn(B, 1, generator=gen) * 2).to(dev)
            h = torch.randn(B, 2, generator=gen).to(dev)
            w = (0.5 + torch.rand(B, K, generator=gen)).to(dev)
            with torch.no_grad():
                out = m.net(h)
                coef = (w * torch.exp(out[:, K:])).contiguous()
                t = (coef * I.hip_forward_multi(spec, None, x, h, n)[0]).sum(1, keepdim=True)
                y = t + (w * out[:, :K]).sum(1, keepdim=True)

                def kernel():
                    return I.hip_solve_multi(spec, h, t, coef, n, lo, hi, tol, max_iter)

                def host_loop():
                    return I.newton_solve_sum(I.quadrature_eval(spec, None, h, n, True), t, coef, lo, hi, tol, max_iter)

                def api():
                    return m.inverse_sum(y, h, w, (lo, hi), tol, max_iter)

                variants = {"kernel": kernel, "host_loop": host_loop, "api": api}
                counts, results = {}, {}
                for name, fn in variants.items():
                    before = launches()
                    results[name] = fn()
                    counts[name] = launches() - before
                kernel()
                kname = _lib.lib().umnn_last_kernel_name().decode()
                for fn in variants.values():
                    for _ in range(args.warmup):
                        fn()
                times = {name: [] for name in variants}
                for _ in range(args.reps):
                    for name, fn in variants.items():
                        times[name].append(wall(fn))
            med = {}
            for name, ts in times.items():
                med[name] = statistics.median(ts)
                emit({"kind": "time", "K": K, "direction": "inverse_sum", "variant": name, "rows": B, "nb_steps": n, "reps": len(ts),
                      "median_ms": med[name], "min_ms": min(ts), "max_ms": max(ts), "mean_ms": statistics.fmean(ts)})
            (xk, _, fk, sk), (xh, _, _, sh) = results["kernel"], results["host_loop"]
            ek, eh = (sk & _lib.SOLVE_EVALS_MASK).float(), (sh & _lib.SOLVE_EVALS_MASK).float()
            D = (coef * fk).sum(1, keepdim=True)
            emit({"kind": "solve", "K": K, "rows": B, "nb_steps": n, "kernel": kname, "quadrature_launches": counts,
                  "evals_per_row_kernel": [float(ek.mean()), float(ek.max())], "evals_per_row_host_loop": [float(eh.mean()), float(eh.max())],
                  "flagged_rows_kernel": int((sk & ~_lib.SOLVE_EVALS_MASK != 0).sum()),
                  "max_x_gap_in_stop_bounds": float(((xk - xh).abs() * D / (tol * t.abs().clamp(min=1.))).max()),
                  "kernel_over_host_loop": med["kernel"] / med["host_loop"], "kernel_not_slower": med["kernel"] <= med["host_loop"]})


if __name__ == "__main__":
    main()
