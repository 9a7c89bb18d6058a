#!/usr/bin/env python
"""Staged Picard tree (torch f and g) against the fused kernel on the same problem: Grad_Dependent_Nonlinear re-declared with eq_id = None,
torch_callbacks = True and torch f / g, against MLP on the registered class.  Wall time per uz_solve (warm-up, then the median of --reps),
then one profiled solve per path with HIP events per phase (PicardEngine.profile), and the largest difference between the two results.
    python tools/staged_vs_fused.py [--d 100] [--n 3] [--rho 3] [--B 16384] [--reps 5] [--warmup 2]"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--d", type=int, default=100)
    ap.add_argument("--n", type=int, default=3)
    ap.add_argument("--rho", type=int, default=3)
    ap.add_argument("--B", type=int, default=16384)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    args = ap.parse_args()
    import numpy as np
    import torch
    from scasml_gp_amd.equations.equations import Grad_Dependent_Nonlinear
    from scasml_gp_amd.solvers.MLP import MLP

    class Twin(Grad_Dependent_Nonlinear):
        eq_id = None
        torch_callbacks = True

        def f(self, x_t, u, z):
            return self.sigma() * u * z.sum(dim=1, keepdim=True)

        def g(self, x_t):
            return 1 - 1 / (1 + torch.exp(x_t[:, -1:] + x_t[:, :-1].sum(dim=1, keepdim=True)))

    d, B = args.d, args.B
    rng = np.random.default_rng(0)
    xt = torch.from_numpy(np.concatenate([rng.uniform(-0.5, 0.5, (B, d)), rng.uniform(0, 0.5, (B, 1))], axis=1).astype(np.float32)).cuda()
    result = {"d": d, "n": args.n, "rho": args.rho, "B": B, "reps": args.reps}
    outs = {}
    for name, eq in (("fused", Grad_Dependent_Nonlinear(d + 1)), ("staged", Twin(d + 1))):
        solver = MLP(eq, seed=0)
        eng = solver._engine
        for _ in range(args.warmup):
            eng.solve(args.n, args.rho, xt, stream_id=0)
        torch.cuda.synchronize()
        times = []
        for _ in range(args.reps):
            t0 = time.perf_counter()
            out, _, _ = eng.solve(args.n, args.rho, xt, stream_id=0)
            torch.cuda.synchronize()
            times.append((time.perf_counter() - t0) * 1e3)
        outs[name] = out.cpu().numpy()
        eng.profile = True
        eng.solve(args.n, args.rho, xt, stream_id=0)
        torch.cuda.synchronize()
        phases = {}
        for pname, e0, e1 in eng._events:                  # summed per phase over the one profiled solve
            phases[pname] = phases.get(pname, 0.0) + e0.elapsed_time(e1)
        eng._events, eng.profile = [], False
        result[name] = {"ms_median": statistics.median(times), "ms_min": min(times), "ms_max": max(times),
                        "phases_ms": {k: round(v, 3) for k, v in sorted(phases.items())}}
    result["staged_over_fused"] = result["staged"]["ms_median"] / result["fused"]["ms_median"]
    result["max_abs_diff"] = float(np.nanmax(np.abs(outs["staged"] - outs["fused"])))
    result["peak_mem_gb"] = torch.cuda.max_memory_allocated() / 1e9
    print(json.dumps(result))


if __name__ == "__main__":
    main()
