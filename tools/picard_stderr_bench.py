#!/usr/bin/env python
"""What the standard-error kernels cost against the plain ones, and the first measured statement of the surrogate's variance reduction.
The two launches of a pair (scasml_picard_tree / scasml_picard_tree_stderr on the same roots and stream) alternate in one process after
warm-up; each launch is bracketed by HIP events (PicardEngine.profile), repeated until each kernel has run for about --window-ms, and the
ratio of the medians is reported with the spread (quartiles) of both.  Shapes: MLP and the ScaSML ACCUMULATE pass at d = 100, n = rho = 3,
B = 16384 (the headline surrogate: bench.py's 1000 + 200 training points, compat = reference), and MLP_full_history at n = 4, M = 3.
Also the median standard error of MLP and of ScaSML on the same roots.  One JSON line, written to profiles/picard_stderr.json as well.
    python tools/picard_stderr_bench.py [--B 16384] [--window-ms 1000] [--max-reps 1000] [--out profiles/picard_stderr.json]"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def quartiles(v):
    q = np.percentile(np.asarray(v, dtype=np.float64), [25, 50, 75])
    return {"median_ms": round(float(q[1]), 4), "q25_ms": round(float(q[0]), 4), "q75_ms": round(float(q[2]), 4), "min_ms": round(float(min(v)), 4)}


def pair(torch, wl, plain_name, stderr_name, window_ms, max_reps, warmup=3):
    """Alternate the plain and the standard-error solve of workload ``wl``; HIP-event durations of the two named kernels."""
    eng = wl.eng

    def run(stderr):
        return eng.solve(wl.n, wl.par, wl.x_dev, stream_id=1, stderr=stderr)
    for _ in range(warmup):
        run(False)
        run(True)
    torch.cuda.synchronize()
    eng.profile, eng._events = True, []
    run(False)
    torch.cuda.synchronize()
    first = [e0.elapsed_time(e1) for name, e0, e1 in eng._events if name == plain_name][0]
    reps = int(max(10, min(max_reps, np.ceil(window_ms / max(first, 1e-3)))))
    eng._events = []
    for _ in range(reps):
        run(False)
        run(True)
    torch.cuda.synchronize()
    times = {plain_name: [], stderr_name: []}
    for name, e0, e1 in eng._events:
        if name in times:
            times[name].append(e0.elapsed_time(e1))
    eng.profile, eng._events = False, []
    a, b = run(False), run(True)
    assert torch.equal(a[0], b[0]), "(u, z) of the standard-error launch differs from the plain launch"
    rec = {"reps": reps, "plain": quartiles(times[plain_name]), "stderr": quartiles(times[stderr_name])}
    rec["ratio_of_medians"] = round(rec["stderr"]["median_ms"] / rec["plain"]["median_ms"], 4)
    rec["median_se"] = float(b[3].median())
    rec["median_abs_u"] = float(b[0][:, 0].abs().median())
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", type=int, default=1 << 14)
    ap.add_argument("--window-ms", type=float, default=1000.0)
    ap.add_argument("--max-reps", type=int, default=1000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "picard_stderr.json"))
    args = ap.parse_args()
    import torch
    import bench
    from scasml_gp_amd import _lib
    from scasml_gp_amd.equations.equations import Grad_Dependent_Nonlinear
    _lib.require_gpu()
    d = 100
    eq = Grad_Dependent_Nonlinear(d + 1)
    eq.geometry()
    x_dom, x_bdy, _ = bench.harness_sets(eq, 1000, 200)
    gp, _ = bench.fit_surrogate(eq, x_dom, x_bdy, "reference")
    result = {"device": torch.cuda.get_device_name(0), "d": d, "B": args.B, "window_ms": args.window_ms}
    mlp = bench.Workload(eq, None, "mlp", "quad", 3, 3, args.B, 0)
    result["mlp_n3_rho3"] = pair(torch, mlp, "picard_mlp", "picard_mlp_stderr", args.window_ms, args.max_reps)
    sca = bench.Workload(eq, gp, "scasml", "quad", 3, 3, args.B, 0)
    result["scasml_accumulate_n3_rho3"] = pair(torch, sca, "picard_accumulate", "picard_accumulate_stderr", args.window_ms, args.max_reps)
    fh = bench.Workload(eq, None, "mlp", "fh", 4, 3, args.B, 0)
    result["mlp_full_history_n4_M3"] = pair(torch, fh, "picard_mlp", "picard_mlp_stderr", args.window_ms, args.max_reps)
    # the same roots (Workload.synth seeds by rank): what the surrogate does to the Monte-Carlo error of the estimate
    result["median_se_mlp"] = result["mlp_n3_rho3"]["median_se"]
    result["median_se_scasml"] = result["scasml_accumulate_n3_rho3"]["median_se"]
    result["se_ratio_mlp_over_scasml"] = round(result["median_se_mlp"] / result["median_se_scasml"], 3)
    line = json.dumps(result)
    print(line)
    with open(args.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
