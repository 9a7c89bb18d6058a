#!/usr/bin/env python
"""What the kernels that estimate the standard errors of u AND z cost (scasml_picard_tree_stderr_uz), against the two launches that exist
beside them: the plain one and the u-only standard-error one.  The three launches of a shape (the same roots, the same stream) alternate in
one process after warm-up; each is bracketed by HIP events (PicardEngine.profile) and repeated until the plain kernel has run for about
--window-ms; medians, quartiles and the ratios of the medians are reported.  Shapes, as tools/picard_stderr_bench.py: MLP and the ScaSML
ACCUMULATE pass at d = 100, n = rho = 3, B = 16384 (the headline surrogate: bench.py's 1000 + 200 training points, compat = reference),
and MLP_full_history at n = 4, M = 3.  Beside the times, on the same roots: the median se of u, the median se of a z component and the
share of the returned z components that sit on the clip.  One JSON line, written to profiles/picard_stderr_uz.json as well.
    python tools/picard_stderr_uz_bench.py [--B 16384] [--window-ms 1000] [--max-reps 1000] [--out profiles/picard_stderr_uz.json]"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from picard_stderr_bench import quartiles  # noqa: E402

MODES = (("plain", False, ""), ("stderr_u", True, "_stderr"), ("stderr_uz", "uz", "_stderr_uz"))


def triple(torch, wl, kernel, window_ms, max_reps, warmup=3):
    """Alternate the three solves of workload ``wl``; HIP-event durations of ``kernel`` (+ "_stderr", + "_stderr_uz")."""
    eng = wl.eng

    def run(stderr):
        return eng.solve(wl.n, wl.par, wl.x_dev, stream_id=1, stderr=stderr)
    for _ in range(warmup):
        for _, stderr, _ in MODES:
            run(stderr)
    torch.cuda.synchronize()
    eng.profile, eng._events = True, []
    run(False)
    torch.cuda.synchronize()
    first = [e0.elapsed_time(e1) for name, e0, e1 in eng._events if name == kernel][0]
    reps = int(max(10, min(max_reps, np.ceil(window_ms / max(first, 1e-3)))))
    eng._events = []
    for _ in range(reps):
        for _, stderr, _ in MODES:
            run(stderr)
    torch.cuda.synchronize()
    times = {kernel + suffix: [] for _, _, suffix in MODES}
    for name, e0, e1 in eng._events:
        if name in times:
            times[name].append(e0.elapsed_time(e1))
    eng.profile, eng._events = False, []
    plain, u_only, uz = (run(stderr) for _, stderr, _ in MODES)
    assert torch.equal(plain[0], uz[0]), "(u, z) of the (u, z) standard-error launch differs from the plain launch"
    assert torch.equal(u_only[3], uz[3][:, 0]), "se of u differs between the two standard-error launches"
    rec = {"reps": reps}
    for label, _, suffix in MODES:
        rec[label] = quartiles(times[kernel + suffix])
    rec["uz_over_plain"] = round(rec["stderr_uz"]["median_ms"] / rec["plain"]["median_ms"], 4)
    rec["uz_over_u_only"] = round(rec["stderr_uz"]["median_ms"] / rec["stderr_u"]["median_ms"], 4)
    rec["u_only_over_plain"] = round(rec["stderr_u"]["median_ms"] / rec["plain"]["median_ms"], 4)
    z, se = uz[0][:, 1:], uz[3]
    rec["median_se_u"] = float(se[:, 0].median())
    rec["median_se_z"] = float(se[:, 1:].median())
    rec["median_abs_z"] = float(z.abs().median())
    rec["clip"] = float(eng.problem().clip)
    rec["share_of_z_on_the_clip"] = round(float((z.abs() >= rec["clip"]).float().mean()), 4)
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", type=int, default=1 << 14)
    ap.add_argument("--window-ms", type=float, default=1000.0)
    ap.add_argument("--max-reps", type=int, default=1000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "picard_stderr_uz.json"))
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
    result["mlp_n3_rho3"] = triple(torch, mlp, "picard_mlp", args.window_ms, args.max_reps)
    sca = bench.Workload(eq, gp, "scasml", "quad", 3, 3, args.B, 0)
    result["scasml_accumulate_n3_rho3"] = triple(torch, sca, "picard_accumulate", args.window_ms, args.max_reps)
    fh = bench.Workload(eq, None, "mlp", "fh", 4, 3, args.B, 0)
    result["mlp_full_history_n4_M3"] = triple(torch, fh, "picard_mlp", args.window_ms, args.max_reps)
    line = json.dumps(result)
    print(line)
    with open(args.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
