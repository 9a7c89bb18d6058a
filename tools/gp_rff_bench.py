#!/usr/bin/env python
"""Time the pathwise posterior draws at d = 100, 1000 + 200 collocation points (M = 4200, Mp = 4224), F = 2048 features:
  (1) the prior kernel scasml_gp_rff_functionals at (n, S) in {1200, 16384} x {1, 64} against the composed torch route on the same features: Omega
      (S x F x (d+1) float64) materialised in HBM beforehand, then per draw float64 x @ Omega^T, cos / sin, P and Q, four weighted reductions;
      and the same kernel at d = 1 (K = 2: no matrix work and one Philox stage to speak of, the same sincos) as the floor of its epilogue;
  (2) a whole GPFunctionDraws.predict by parts (prior kernel, scasml_gp_cross_rows op 0, scasml_gemm_nt_sub) and GP.sample_functions (its set-up)
      against GP.sample_posterior at n = 1200 and 4096, S = 64.
HIP events around each part, 3 warm-ups, median of 20 runs, the routes alternating inside one process.  Writes profiles/gp_rff_d100.json.
    python tools/gp_rff_bench.py [reps] [out.json]"""
import functools
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
WARMUPS = 3
reps = int(sys.argv[1]) if len(sys.argv) > 1 else 20
out_path = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "profiles", "gp_rff_d100.json")
d, nd, nb, F, SEED = 100, 1000, 200, 2048, 7
lib = _lib.load()
_lib.require_gpu()
s = _lib.stream_ptr()


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


def run(parts):
    """parts: ordered {name: fn}; the first WARMUPS rounds are dropped."""
    got = {k: [] for k in parts}
    for r in range(WARMUPS + reps):
        for k, fn in parts.items():
            t = timed(fn)
            if r >= WARMUPS:
                got[k].append(t)
    return {k: {"median_ms": statistics.median(v), "best_ms": min(v), "runs_ms": v} for k, v in got.items()}


def rff(dim, a, X, S, out):
    _lib.check(lib.scasml_gp_rff_functionals(dim, a, _lib.ptr(X), X.shape[0], X.stride(0), F, SEED, 0, S, _lib.ptr(out), s), "gp_rff_functionals")


@functools.lru_cache(maxsize=None)
def features(dim, a, S):
    """(Omega (S, F, dim+1), wc (S, F), ws (S, F)) float64 on the device: the kernel's own features, from the oracle's Philox statement."""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import _gp_rff_ref as ref
    v = torch.from_numpy(ref.feature_normals(dim, SEED, np.arange(S), F).astype(np.float64)).cuda()
    return (np.sqrt(a) * v[:, :, :dim + 1]).contiguous(), v[:, :, dim + 1].contiguous(), v[:, :, dim + 2].contiguous()


rng = np.random.default_rng(0)
dom = np.concatenate([rng.uniform(-0.5, 0.5, (nd, d)), rng.uniform(0.0, 0.5, (nd, 1))], axis=1).astype(np.float32)
bdy = np.concatenate([rng.uniform(-0.5, 0.5, (nb, d)), rng.uniform(0.0, 0.5, (nb, 1))], axis=1).astype(np.float32)
bdy[np.arange(nb), rng.integers(0, d, nb)] = 0.5
gp = GP_Grad_Dependent_Nonlinear(Grad_Dependent_Nonlinear(d + 1), compat=None)
gp.load_right_vector(dom, bdy, 1e-3 * rng.standard_normal(4 * nd + nb))
z = rng.standard_normal(4 * nd + nb)
a = gp.a
result = {"d": d, "n_domain": nd, "n_boundary": nb, "M": 4 * nd + nb, "F": F, "reps": reps, "warmups": WARMUPS, "fp64_mfma_peak_tflops": PEAK_TFLOPS,
          "device": torch.cuda.get_device_name(0), "kernel": {}, "predict": {}}
points = {n: torch.from_numpy(np.concatenate([rng.uniform(-0.5, 0.5, (n, d)), rng.uniform(0.0, 0.5, (n, 1))], axis=1).astype(np.float32)).cuda()
          for n in (1200, 4096, 16384)}

# ---- (1) the prior kernel against the composed torch route
for n in (1200, 16384):
    X = points[n]
    X64 = X.double()
    X1 = X[:, -2:].contiguous()                      # the same number of points with d = 1
    for S in (1, 64):
        out, out1, comp = (torch.empty((S, n, 4), dtype=torch.float64, device="cuda") for _ in range(3))
        Om, wc, ws = features(d, a, S)
        mult = torch.stack([torch.ones_like(wc), -(Om[:, :, :d] ** 2).sum(-1), Om[:, :, d], Om[:, :, :d].sum(-1)], dim=-1)      # (S, F, 4)

        def composed():
            for r in range(S):
                theta = X64 @ Om[r].t()
                c, sn = torch.cos(theta), torch.sin(theta)
                P, Q = wc[r] * c + ws[r] * sn, ws[r] * c - wc[r] * sn
                comp[r, :, 0:2] = P @ mult[r, :, 0:2]
                comp[r, :, 2:4] = Q @ mult[r, :, 2:4]
            comp.mul_(F ** -0.5)

        case = run({"kernel": lambda: rff(d, a, X, S, out), "composed_torch": composed, "kernel_d1": lambda: rff(1, a, X1, S, out1)})
        flop = 2.0 * S * n * F * (d + 1)
        case["flop"] = flop
        case["kernel_tflops"] = flop / case["kernel"]["median_ms"] / 1e9
        case["kernel_fraction_of_fp64_mfma_peak"] = case["kernel_tflops"] / PEAK_TFLOPS
        case["sincos_per_second"] = S * n * F / (case["kernel"]["median_ms"] * 1e-3)
        case["omega_bytes_of_the_composed_route"] = Om.numel() * 8
        case["largest_difference_kernel_minus_composed_over_largest_value"] = float((out - comp).abs().max() / comp.abs().max())
        result["kernel"]["n=%d S=%d" % (n, S)] = case
        print("kernel n=%5d S=%2d  %.3f ms = %.2f TFLOP/s = %.3f of peak, %.2e sincos/s | d = 1: %.3f ms | composed torch %.3f ms | difference %.1e" % (
            n, S, case["kernel"]["median_ms"], case["kernel_tflops"], case["kernel_fraction_of_fp64_mfma_peak"], case["sincos_per_second"],
            case["kernel_d1"]["median_ms"], case["composed_torch"]["median_ms"], case["largest_difference_kernel_minus_composed_over_largest_value"]), flush=True)

# ---- (2) a whole predict by parts against sample_posterior
S = 64
draws = gp.sample_functions(S, seed=SEED, n_features=F, z=z)
L = gp._variance_factor()
Mp = L.shape[0]
for n in (1200, 4096):
    X = points[n]
    rows = torch.zeros((n, Mp), dtype=torch.float64, device="cuda")
    prior = torch.empty((S, n, 4), dtype=torch.float64, device="cuda")
    vals = [None]

    def cross():
        gp._cross_rows(gp._xd, gp._xb, 0, X, rows, Mp, 0)

    def transpose():
        vals[0] = prior[:, :, 0].t().contiguous()

    def gemm():
        _lib.check(lib.scasml_gemm_nt_sub(_lib.ptr(vals[0]), S, n, S, _lib.ptr(rows), Mp, _lib.ptr(draws._neg), Mp, Mp, 0, 0, 0, s), "gemm_nt_sub")

    case = run({"prior_kernel": lambda: rff(d, a, X, S, prior), "cross_rows": cross, "transpose": transpose, "gemm_nt_sub": gemm,
                "predict": lambda: draws.predict(X), "sample_functions": lambda: gp.sample_functions(S, seed=SEED, n_features=F, z=z),
                "sample_posterior": lambda: gp.sample_posterior(X, S, seed=SEED)})
    case["parts_reproduce_the_call_bit_for_bit"] = bool(torch.equal(vals[0].t(), draws.predict(X)))
    case["sum_of_parts_ms"] = sum(case[k]["median_ms"] for k in ("prior_kernel", "cross_rows", "transpose", "gemm_nt_sub"))
    result["predict"]["n=%d S=%d" % (n, S)] = case
    print("predict n=%4d S=%d  prior %.2f | cross rows %.2f | transpose %.2f | gemm %.2f ms | sum %.2f, predict %.2f ms | sample_functions %.2f ms | "
          "sample_posterior %.2f ms | same bits %s" % (n, S, case["prior_kernel"]["median_ms"], case["cross_rows"]["median_ms"], case["transpose"]["median_ms"],
                                                       case["gemm_nt_sub"]["median_ms"], case["sum_of_parts_ms"], case["predict"]["median_ms"],
                                                       case["sample_functions"]["median_ms"], case["sample_posterior"]["median_ms"],
                                                       case["parts_reproduce_the_call_bit_for_bit"]), flush=True)
with open(out_path, "w") as f:
    json.dump(result, f, indent=1, sort_keys=True)
    f.write("\n")
