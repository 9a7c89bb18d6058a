#!/usr/bin/env python
"""Time the 4 x 4 posterior covariance of [u, Lap u, dt u, div u] at the reference's shape -- d = 20, 1000 + 200 collocation points (M = 4200,
Mp = 4224) -- at n = 4096 points (16 384 rows), two routes on the same interleaved feature rows:
  (a) the shipped launch: scasml_gp_functional_covariance (solve and the ten inner products of every point in one kernel);
  (b) the composed route: scasml_gp_variance on the 4 n rows (the same solve, the sums of squares alone), then a torch batched product of the solved
      rows, P - V V^T.
HIP events around each part, the rows restored from a pristine copy outside the timed region, 3 warm-ups, median of `reps` runs, the routes alternating
inside one process.  Writes profiles/gp_functional_covariance_timing.json.
    python tools/gp_functional_covariance_bench.py [reps] [out.json]"""
import ctypes as C
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402
from scasml_gp_amd import _lib  # noqa: E402
from scasml_gp_amd.equations.equations import Grad_Dependent_Nonlinear  # noqa: E402
from scasml_gp_amd.models.GP import GP_Grad_Dependent_Nonlinear  # noqa: E402

reps = int(sys.argv[1]) if len(sys.argv) > 1 else 20
out_path = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "profiles", "gp_functional_covariance_timing.json")
WARMUP = 3
d, nd, nb, n = 20, 1000, 200, 4096
lib = _lib.load()
_lib.require_gpu()


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


def summary(ms):
    return {"best_ms": min(ms), "median_ms": statistics.median(ms), "runs_ms": ms}


rng = np.random.default_rng(0)
dom = np.concatenate([rng.uniform(-0.5, 0.5, (nd, d)), rng.uniform(0.0, 0.5, (nd, 1))], axis=1).astype(np.float32)
bdy = np.concatenate([rng.uniform(-0.5, 0.5, (nb, d)), rng.uniform(0.0, 0.5, (nb, 1))], axis=1).astype(np.float32)
bdy[np.arange(nb), rng.integers(0, d, nb)] = 0.5
gp = GP_Grad_Dependent_Nonlinear(Grad_Dependent_Nonlinear(d + 1), compat=None)
gp.kernel_phi_phi(dom, bdy)
L = gp._variance_factor()
Mp = L.shape[0]
X = torch.from_numpy(np.concatenate([rng.uniform(-0.5, 0.5, (n, d)), rng.uniform(0.0, 0.5, (n, 1))], axis=1).astype(np.float32)).cuda()
pristine = torch.zeros((n, 4, Mp), dtype=torch.float64, device="cuda")
for o in range(4):
    gp._cross_rows(gp._xd, gp._xb, o, X, pristine[:, o, :], 4 * Mp, 0)
rows = torch.empty_like(pristine)
prior_h = np.ascontiguousarray(gp._functional_prior())
prior_d = torch.from_numpy(prior_h).cuda()
cov_new = torch.empty((n, 4, 4), dtype=torch.float64, device="cuda")
var = torch.empty(4 * n, dtype=torch.float64, device="cuda")
cov_composed = [None]
s = _lib.stream_ptr()


def fused():
    _lib.check(lib.scasml_gp_functional_covariance(_lib.ptr(L), Mp, _lib.ptr(rows), Mp, n, prior_h.ctypes.data_as(C.c_void_p), _lib.ptr(cov_new), s),
               "gp_functional_covariance")


def solve():
    _lib.check(lib.scasml_gp_variance(_lib.ptr(L), Mp, _lib.ptr(rows), Mp, 4 * n, 1.0, _lib.ptr(var), s), "gp_variance")


def product():
    cov_composed[0] = prior_d[None] - torch.bmm(rows, rows.transpose(1, 2))


parts = {"functional_covariance_kernel": [], "composed_variance_kernel": [], "composed_batched_product": []}
for r in range(WARMUP + reps):
    rows.copy_(pristine)
    t = {"functional_covariance_kernel": timed(fused)}
    rows.copy_(pristine)
    t["composed_variance_kernel"] = timed(solve)
    t["composed_batched_product"] = timed(product)
    if r >= WARMUP:
        for k, v in t.items():
            parts[k].append(v)
scale = torch.sqrt(torch.diagonal(prior_d))
diff = float(((cov_new - cov_composed[0]).abs() / (scale[:, None] * scale[None, :])).max())
result = {"d": d, "n_domain": nd, "n_boundary": nb, "M": 4 * nd + nb, "Mp": Mp, "n_points": n, "rows": 4 * n, "reps": reps, "warmup": WARMUP,
          "device": torch.cuda.get_device_name(0)}
result.update({k: summary(v) for k, v in parts.items()})
result["new_launch_median_ms"] = result["functional_covariance_kernel"]["median_ms"]
result["composed_route_median_ms"] = result["composed_variance_kernel"]["median_ms"] + result["composed_batched_product"]["median_ms"]
result["scaled_max_difference_of_the_two_routes"] = diff
print("d=%d M=%d n=%d: new launch %.2f ms | composed: variance kernel on 4n rows %.2f + batched product %.2f = %.2f ms (medians of %d) | scaled max "
      "|difference| %.2e" % (d, 4 * nd + nb, n, result["new_launch_median_ms"], result["composed_variance_kernel"]["median_ms"],
                             result["composed_batched_product"]["median_ms"], result["composed_route_median_ms"], reps, diff), flush=True)
with open(out_path, "w") as f:
    json.dump(result, f, indent=1, sort_keys=True)
    f.write("\n")
