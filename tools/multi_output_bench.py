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
    for K in [int(k) for k in args.only_k.split(",")]:
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


if __name__ == "__main__":
    main()
