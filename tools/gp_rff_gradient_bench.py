#!/usr/bin/env python
"""Time the per-component gradients of the pathwise posterior draws at d = 100, 1000 + 200 collocation points (M = 4200, Mp = 4224), F = 2048:
  (1) the prior kernel scasml_gp_rff_gradient at (n, S) in {1200, 16384} x {1, 64} against scasml_gp_rff_functionals at the same shape (the same
      theta product and sincos, four running sums instead of the second product) and against the composed torch float64 route on features
      materialised in HBM beforehand: per draw x @ Omega^T, cos / sin, Q, Q @ Omega; and the same kernel at d = 1 (K = 2, one component tile of two
      components: the sincos, Q through LDS and one second-product tile, next to no Philox) and at d = 63 (one full component tile) as its floors;
  (2) a whole GPFunctionDraws.gradient by parts at n = 1200, S in {1, 64}: the prior kernel, the two scasml_gp_cross_rows calls (op 2, op 0), the
      two scasml_gemm_nt_sub calls on them, and the alpha pass (elementwise torch, one scasml_gemm_nt_sub and the assembly per draw).
HIP events around each part, 3 warm-ups, median of 20 runs, the routes alternating inside one process.  Writes profiles/gp_rff_gradient_d100.json.
    python tools/gp_rff_gradient_bench.py [reps] [out.json]"""
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402
import torch  # noqa: E402
import _gp_rff_ref as ref  # noqa: E402
from scasml_gp_amd import _lib  # noqa: E402
from scasml_gp_amd.equations.equations import Grad_Dependent_Nonlinear  # noqa: E402
from scasml_gp_amd.models.GP import GP_Grad_Dependent_Nonlinear  # noqa: E402

PEAK_TFLOPS = 78.6
WARMUPS = 3
reps = int(sys.argv[1]) if len(sys.argv) > 1 else 20
out_path = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "profiles", "gp_rff_gradient_d100.json")
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


rng = np.random.default_rng(0)
dom = np.concatenate([rng.uniform(-0.5, 0.5, (nd, d)), rng.uniform(0.0, 0.5, (nd, 1))], axis=1).astype(np.float32)
bdy = np.concatenate([rng.uniform(-0.5, 0.5, (nb, d)), rng.uniform(0.0, 0.5, (nb, 1))], axis=1).astype(np.float32)
bdy[np.arange(nb), rng.integers(0, d, nb)] = 0.5
gp = GP_Grad_Dependent_Nonlinear(Grad_Dependent_Nonlinear(d + 1), compat=None)
gp.load_right_vector(dom, bdy, 1e-3 * rng.standard_normal(4 * nd + nb))
z = rng.standard_normal(4 * nd + nb)
a = gp.a
result = {"d": d, "n_domain": nd, "n_boundary": nb, "M": 4 * nd + nb, "F": F, "reps": reps, "warmups": WARMUPS, "fp64_mfma_peak_tflops": PEAK_TFLOPS,
          "device": torch.cuda.get_device_name(0), "kernel": {}, "gradient": {}}
points = {n: torch.from_numpy(np.concatenate([rng.uniform(-0.5, 0.5, (n, d)), rng.uniform(0.0, 0.5, (n, 1))], axis=1).astype(np.float32)).cuda()
          for n in (1200, 16384)}
v64 = torch.from_numpy(ref.feature_normals(d, SEED, np.arange(64), F).astype(np.float64)).cuda()      # the kernel's own features, from the oracle's Philox statement

# ---- (1) the prior kernel against the functionals kernel and the composed torch route
for n in (1200, 16384):
    X = points[n]
    X64 = X.double()
    X1, X63 = X[:, -2:].contiguous(), X[:, -64:].contiguous()              # the same number of points with d = 1 and d = 63
    for S in (1, 64):
        out1, out63 = torch.empty((S, n, 2), dtype=torch.float64, device="cuda"), torch.empty((S, n, 64), dtype=torch.float64, device="cuda")
        out, comp = (torch.empty((S, n, d + 1), dtype=torch.float64, device="cuda") for _ in range(2))
        fun = torch.empty((S, n, 4), dtype=torch.float64, device="cuda")
        Om, wc, ws = (np.sqrt(a) * v64[:S, :, :d + 1]).contiguous(), v64[:S, :, d + 1].contiguous(), v64[:S, :, d + 2].contiguous()

        def kernel(dim=d, pts=X, res=out):
            _lib.check(lib.scasml_gp_rff_gradient(dim, a, _lib.ptr(pts), n, pts.stride(0), F, SEED, 0, S, _lib.ptr(res), dim + 1, s), "gp_rff_gradient")

        def functionals():
            _lib.check(lib.scasml_gp_rff_functionals(d, a, _lib.ptr(X), n, X.stride(0), F, SEED, 0, S, _lib.ptr(fun), s), "gp_rff_functionals")

        def composed():
            for r in range(S):
                theta = X64 @ Om[r].t()
                comp[r] = (ws[r] * torch.cos(theta) - wc[r] * torch.sin(theta)) @ Om[r]
            comp.mul_(F ** -0.5)

        case = run({"kernel": kernel, "functionals_kernel": functionals, "composed_torch": composed,
                    "kernel_d1": lambda: kernel(1, X1, out1), "kernel_d63": lambda: kernel(63, X63, out63)})
        flop = 2.0 * 2.0 * S * n * F * (d + 1)                  # the two products
        case["flop"] = flop
        case["kernel_tflops"] = flop / case["kernel"]["median_ms"] / 1e9
        case["kernel_fraction_of_fp64_mfma_peak"] = case["kernel_tflops"] / PEAK_TFLOPS
        case["sincos_per_second"] = S * n * F / (case["kernel"]["median_ms"] * 1e-3)
        case["kernel_over_functionals_kernel"] = case["kernel"]["median_ms"] / case["functionals_kernel"]["median_ms"]
        case["omega_bytes_of_the_composed_route"] = Om.numel() * 8
        case["largest_difference_kernel_minus_composed_over_largest_value"] = float((out - comp).abs().max() / comp.abs().max())
        result["kernel"]["n=%d S=%d" % (n, S)] = case
        print("kernel n=%5d S=%2d  %.3f ms = %.2f TFLOP/s = %.3f of peak, %.2e sincos/s | functionals kernel %.3f ms (x %.2f) | composed torch %.3f ms | "
              "d = 1: %.3f ms, d = 63: %.3f ms | difference %.1e" % (n, S, case["kernel"]["median_ms"], case["kernel_tflops"],
                                   case["kernel_fraction_of_fp64_mfma_peak"], case["sincos_per_second"],
                                   case["functionals_kernel"]["median_ms"], case["kernel_over_functionals_kernel"], case["composed_torch"]["median_ms"],
                                   case["kernel_d1"]["median_ms"], case["kernel_d63"]["median_ms"],
                                   case["largest_difference_kernel_minus_composed_over_largest_value"]), flush=True)

# ---- (2) a whole gradient by parts (the steps of GP._data_gradient, one chunk)
n = 1200
X = points[n]
N, Nb, M = nd, nb, 4 * nd + nb
for S in (1, 64):
    draws = gp.sample_functions(S, seed=SEED, n_features=F, z=z)
    neg = draws._neg
    Mp, Np = neg.shape[1], (N + Nb + 31) // 32 * 32
    f64 = dict(dtype=torch.float64, device="cuda")
    rows2, rows0 = torch.zeros((n, Mp), **f64), torch.zeros((n, Mp), **f64)
    prior, tail, grad = torch.empty((S, n, d + 1), **f64), torch.zeros((n, 2, S), **f64), torch.empty((S, n, d + 1), **f64)
    yext = torch.zeros((d + 1, Np), **f64)
    yext[:d, :N], yext[:d, N:N + Nb], yext[d, :N + Nb] = gp._xd[:, :d].t(), gp._xb[:, :d].t(), 1.0
    neg_div = torch.zeros((S, Mp), **f64)
    neg_div[:, :N] = a * neg[:, 3 * N + Nb:4 * N + Nb]
    x64 = X[:, :d].double()

    def prior_kernel():
        _lib.check(lib.scasml_gp_rff_gradient(d, a, _lib.ptr(X), n, X.stride(0), F, SEED, 0, S, _lib.ptr(prior), d + 1, s), "gp_rff_gradient")

    def cross():
        gp._cross_rows(gp._xd, gp._xb, 2, X, rows2, Mp, 0)
        gp._cross_rows(gp._xd, gp._xb, 0, X, rows0, Mp, 0)

    def tails():
        tail.zero_()
        gp._gemm_nt_sub(tail[:, 0, :], rows2, Mp, neg, Mp)
        gp._gemm_nt_sub(tail[:, 1, :], rows0, Mp, neg_div, Mp)

    def alpha_pass():
        gp._gradient_alpha_pass(rows0, x64, neg, yext, tail, grad)
        grad.add_(prior)

    case = run({"prior_kernel": prior_kernel, "cross_rows_op2_op0": cross, "tail_gemms": tails, "alpha_pass": alpha_pass,
                "gradient": lambda: draws.gradient(X), "functionals": lambda: draws.functionals(X)})
    case["parts_reproduce_the_call_bit_for_bit"] = bool(torch.equal(grad, draws.gradient(X)))
    case["sum_of_parts_ms"] = sum(case[k]["median_ms"] for k in ("prior_kernel", "cross_rows_op2_op0", "tail_gemms", "alpha_pass"))
    case["op4_rows_bytes_this_avoids"] = n * M * (d + 1) * 8
    result["gradient"]["n=%d S=%d" % (n, S)] = case
    print("gradient n=%4d S=%2d  prior %.2f | cross rows %.2f | tail gemms %.2f | alpha pass %.2f ms | sum %.2f, gradient %.2f ms | functionals %.2f ms | "
          "same bits %s" % (n, S, case["prior_kernel"]["median_ms"], case["cross_rows_op2_op0"]["median_ms"], case["tail_gemms"]["median_ms"],
                            case["alpha_pass"]["median_ms"], case["sum_of_parts_ms"], case["gradient"]["median_ms"], case["functionals"]["median_ms"],
                            case["parts_reproduce_the_call_bit_for_bit"]), flush=True)
with open(out_path, "w") as f:
    json.dump(result, f, indent=1, sort_keys=True)
    f.write("\n")
