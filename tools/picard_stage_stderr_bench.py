#!/usr/bin/env python
"""What the standard errors of a callback equation cost (scasml_picard_stage_stderr, PicardEngine._solve_staged).  Two comparisons at each
shape, the two sides alternating in one process after warm-up, every interval bracketed by HIP events, medians and quartiles over a window:
  the whole staged solve, plain against return_stderr="uz" (GENERATE, the callbacks, the gathers and scatters, every stage);
  the last-stage launch alone, plain against standard-error (PicardEngine.profile's events inside those same solves).
The plain solve runs the code it ran before the estimate existed (the plain kernel instances are unchanged), so the ratios are against that.
Shapes: d = 100, 16384 roots, the torch equation f = -u sin(x_0 + t) + mean(a_i z_i^2), g = cos(2 sum x_i); quadrature n = rho = 3 and full
history n = 4, M = 3 -- those of tools/picard_stderr_uz_bench.py, whose fused MLP kernels paid 1.08 and 1.16 for the same accumulators.  One JSON
line, written to profiles/picard_stage_stderr.json as well.
    python tools/picard_stage_stderr_bench.py [--B 16384] [--window-ms 1000] [--max-reps 200] [--out profiles/picard_stage_stderr.json]"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from picard_stderr_bench import quartiles  # noqa: E402


def steep(torch, d):
    from scasml_gp_amd.equations.equations import Equation

    class Steep(Equation):
        eq_id = None
        torch_callbacks = True
        staged_stderr = True

        def __init__(self, n_input):
            super().__init__(n_input)
            self.norm_estimation = 1.0
            self.uncertainty = 0.1
            self.a = torch.tensor(0.5 + np.arange(n_input - 1) / max(n_input - 2, 1), dtype=torch.float32, device="cuda")

        def geometry(self, t0=0, T=0.5):
            self.t0, self.T = t0, T

        def mu(self, x_t=0):
            return 0.1

        def sigma(self, x_t=0):
            return 0.25

        def f(self, x_t, u, z):
            return -u * torch.sin(x_t[:, :1] + x_t[:, -1:]) + (self.a * z * z).mean(dim=1, keepdim=True)

        def g(self, x_t):
            return torch.cos(2.0 * x_t[:, :-1].sum(dim=1, keepdim=True))
    return Steep(d + 1)


def measure(torch, solver, n, par, x, window_ms, max_reps, warmup=2):
    eng = solver._engine
    last = "picard_staged_stage%d" % n

    def run(stderr):
        return eng.solve(n, par, x, stream_id=1, stderr=stderr)
    for _ in range(warmup):
        run(False)
        run("uz")
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    run(False)
    e1.record()
    torch.cuda.synchronize()
    reps = int(max(5, min(max_reps, np.ceil(window_ms / max(e0.elapsed_time(e1), 1e-3)))))
    eng.profile, eng._events = True, []
    whole = {False: [], "uz": []}
    for _ in range(reps):
        for stderr in (False, "uz"):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            run(stderr)
            b.record()
            whole[stderr].append((a, b))
    torch.cuda.synchronize()
    per = {}
    for name, a, b in eng._events:
        per.setdefault(name, []).append(a.elapsed_time(b))
    eng.profile, eng._events = False, []
    plain, uz = run(False), run("uz")
    assert torch.equal(plain[0], uz[0]), "(u, z) of the standard-error solve differs from the plain solve"
    rec = {"reps": reps,
           "solve_plain": quartiles([a.elapsed_time(b) for a, b in whole[False]]),
           "solve_stderr_uz": quartiles([a.elapsed_time(b) for a, b in whole["uz"]]),
           "last_stage_plain": quartiles(per[last]),
           "last_stage_stderr": quartiles(per[last + "_stderr"])}
    rec["solve_ratio"] = round(rec["solve_stderr_uz"]["median_ms"] / rec["solve_plain"]["median_ms"], 4)
    rec["last_stage_ratio"] = round(rec["last_stage_stderr"]["median_ms"] / rec["last_stage_plain"]["median_ms"], 4)
    # where a solve's time goes: every bracketed interval summed per name and divided by the solves the name occurs in (the last stage's two
    # names in `reps` solves each, every other name in both kinds of solve)
    rec["per_solve_ms"] = {k: round(float(np.sum(v)) / (reps if k in (last, last + "_stderr") else 2 * reps), 4) for k, v in sorted(per.items())}
    se = uz[3]
    rec["median_se_u"], rec["median_se_z"] = float(se[:, 0].median()), float(se[:, 1:].median())
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", type=int, default=1 << 14)
    ap.add_argument("--window-ms", type=float, default=1000.0)
    ap.add_argument("--max-reps", type=int, default=200)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "picard_stage_stderr.json"))
    args = ap.parse_args()
    import torch
    from oracle.equation import sample_points
    from scasml_gp_amd import _lib
    from scasml_gp_amd.solvers.MLP import MLP
    from scasml_gp_amd.solvers.MLP_full_history import MLP_full_history
    _lib.require_gpu()
    d = 100
    xt = np.concatenate(sample_points(np.random.default_rng(5), d, args.B - args.B // 4, args.B // 4)).astype(np.float32)
    x = torch.from_numpy(xt).cuda()
    result = {"device": torch.cuda.get_device_name(0), "d": d, "B": args.B, "window_ms": args.window_ms,
              "fused_uz_over_plain": {"mlp_n3_rho3": 1.08, "mlp_full_history_n4_M3": 1.16}}        # profiles/picard_stderr_uz.json
    result["mlp_n3_rho3"] = measure(torch, MLP(steep(torch, d)), 3, 3, x, args.window_ms, args.max_reps)
    result["mlp_full_history_n4_M3"] = measure(torch, MLP_full_history(steep(torch, d)), 4, 3, x, args.window_ms, args.max_reps)
    line = json.dumps(result)
    print(line)
    with open(args.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
