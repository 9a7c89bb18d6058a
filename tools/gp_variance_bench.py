#!/usr/bin/env python
"""Time GP.predict_variance's device work at d = 100, 1000 + 200 collocation points (M = 4200, Mp = 4224), n = 1200 and 16 384, both surrogates:
  (a) the shipped path, split into its two launches: feature rows (scasml_gp_cross_rows, op 0) and scasml_gp_variance;
  (b) the route the ABI allowed before that entry point: feature rows -> transpose into (Mp x n) -> scasml_trsm_lower(trans = 0, nrhs = n) ->
      torch square-sum.
HIP events around each part, every shape warmed up, best and median of `reps` runs, (a) and (b) alternating inside one process.  Writes
profiles/gp_variance_d100.json: the times, the kernel's FP64 TFLOP/s against n Mp^2 flop and its fraction of the 78.6 TFLOP/s FP64-MFMA peak
DESIGN.md uses.
    python tools/gp_variance_bench.py [reps] [out.json]"""
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

PEAK_TFLOPS = 78.6
reps = int(sys.argv[1]) if len(sys.argv) > 1 else 5
out_path = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "profiles", "gp_variance_d100.json")
d, nd, nb = 100, 1000, 200
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
dom = np.concatenate([rng.uniform(-0.5, 0.5, (nd, d)), rng.uniform(0.0, 0.5, (nd, 1))], axis=1).astype(np.float16).astype(np.float32)
bdy = np.concatenate([rng.uniform(-0.5, 0.5, (nb, d)), rng.uniform(0.0, 0.5, (nb, 1))], axis=1).astype(np.float16).astype(np.float32)
bdy[np.arange(nb), rng.integers(0, d, nb)] = 0.5
result = {"d": d, "n_domain": nd, "n_boundary": nb, "M": 4 * nd + nb, "reps": reps, "fp64_mfma_peak_tflops": PEAK_TFLOPS, "device": torch.cuda.get_device_name(0),
          "cases": {}}
for compat in (None, "reference"):
    gp = GP_Grad_Dependent_Nonlinear(Grad_Dependent_Nonlinear(d + 1), compat=compat)
    gp.kernel_phi_phi(dom, bdy)
    L = gp._L_pad
    Mp, M = L.shape[0], gp.phi_dim
    as_coded = compat == "reference"
    idx = gp.laplacian_idx.ctypes.data_as(C.c_void_p) if as_coded else None
    r16 = gp._gram_bits(gp._xd, gp._xb, False) if as_coded else 0
    for n in (1200, 16384):
        X = torch.from_numpy(rng.uniform(-0.5, 0.5, (n, d + 1)).astype(np.float32)).cuda()
        rows = torch.zeros((n, Mp), dtype=torch.float64, device="cuda")
        B = torch.zeros((Mp, n), dtype=torch.float64, device="cuda")
        var = torch.empty(n, dtype=torch.float64, device="cuda")
        s = _lib.stream_ptr()

        def make_rows():
            _lib.check(lib.scasml_gp_cross_rows(d, gp.a, _lib.ptr(gp._xd), nd, _lib.ptr(gp._xb), nb, idx, r16, 0 if as_coded else 1, 0, _lib.ptr(X), n, d + 1,
                                                _lib.ptr(rows), Mp, s), "gp_cross_rows")

        def kernel():
            _lib.check(lib.scasml_gp_variance(_lib.ptr(L), Mp, _lib.ptr(rows), Mp, n, 1.0, _lib.ptr(var), s), "gp_variance")

        def transpose():
            B.copy_(rows.t())

        def solve():
            _lib.check(lib.scasml_trsm_lower(_lib.ptr(L), Mp, _lib.ptr(B), n, 0, s), "trsm_lower")

        composed_var = [None]

        def square_sum():
            composed_var[0] = 1.0 - (B * B).sum(0)

        parts = {"rows": [], "variance_kernel": [], "composed_transpose": [], "composed_trsm_lower": [], "composed_square_sum": []}
        for r in range(reps + 1):                        # run 0 warms every shape up and is dropped
            t = {"rows": timed(make_rows), "composed_transpose": timed(transpose), "composed_trsm_lower": timed(solve), "composed_square_sum": timed(square_sum),
                 "variance_kernel": timed(kernel)}       # the kernel last: it overwrites the rows the composed route copied
            if r:
                for k, v in t.items():
                    parts[k].append(v)
        diff = float((var - composed_var[0]).abs().max())
        case = {k: summary(v) for k, v in parts.items()}
        flop = float(n) * Mp * Mp
        case["flop_n_Mp2"] = flop
        case["variance_kernel_tflops"] = flop / case["variance_kernel"]["best_ms"] / 1e9
        case["variance_kernel_fraction_of_fp64_mfma_peak"] = case["variance_kernel_tflops"] / PEAK_TFLOPS
        case["new_path_ms"] = case["rows"]["best_ms"] + case["variance_kernel"]["best_ms"]
        case["composed_route_ms"] = case["rows"]["best_ms"] + sum(case[k]["best_ms"] for k in ("composed_transpose", "composed_trsm_lower", "composed_square_sum"))
        case["composed_trsm_lower_tflops"] = flop / case["composed_trsm_lower"]["best_ms"] / 1e9
        case["max_abs_difference_of_the_two_routes"] = diff
        result["cases"]["%s n=%d" % (compat or "documented", n)] = case
        print("%-10s n=%5d  rows %.2f ms | variance kernel %.2f ms = %.1f TFLOP/s = %.2f of peak | composed: transpose %.2f + trsm_lower %.2f (%.1f TFLOP/s) + "
              "square-sum %.2f ms | new path %.2f ms, composed route %.2f ms | max |difference| %.2e" % (
                  compat or "documented", n, case["rows"]["best_ms"], case["variance_kernel"]["best_ms"], case["variance_kernel_tflops"],
                  case["variance_kernel_fraction_of_fp64_mfma_peak"], case["composed_transpose"]["best_ms"], case["composed_trsm_lower"]["best_ms"],
                  case["composed_trsm_lower_tflops"], case["composed_square_sum"]["best_ms"], case["new_path_ms"], case["composed_route_ms"], diff), flush=True)
with open(out_path, "w") as f:
    json.dump(result, f, indent=1, sort_keys=True)
    f.write("\n")
