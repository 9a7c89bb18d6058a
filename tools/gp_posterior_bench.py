#!/usr/bin/env python
"""Time the joint-posterior device work at d = 100, 1000 + 200 collocation points (M = 4200, Mp = 4224), n = 1200 and 4096 evaluation points:
  (a) GP.predict_covariance(x), both surrogates, split into its parts: feature rows (scasml_gp_cross_rows, op 0), solve (scasml_gp_variance, rows <- rows
      L^-T), prior block, product (scasml_gemm_nt_sub, lower 256-blocks) + mirror;
  (b) the sampling kernel scasml_gp_sample at S = 64 and 4096 draws on the factor of the documented surrogate's covariance + nugget I, against the
      route the ABI allowed before it: torch.randn (S x np float64 in HBM), the mean broadcast into the output, scasml_gemm_nt_sub on the full square
      (that entry point's triangular map works in 256-row blocks of a factor's panels, not on the B operand's columns).
HIP events around each part, every shape warmed up, best and median of `reps` runs, both routes alternating inside one process.  Writes
profiles/gp_posterior_d100.json.
    python tools/gp_posterior_bench.py [reps] [out.json]"""
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
out_path = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "profiles", "gp_posterior_d100.json")
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


def run(parts):
    """parts: ordered {name: fn}; run 0 warms every shape up and is dropped."""
    got = {k: [] for k in parts}
    for r in range(reps + 1):
        for k, fn in parts.items():
            t = timed(fn)
            if r:
                got[k].append(t)
    return {k: summary(v) for k, v in got.items()}


rng = np.random.default_rng(0)
dom = np.concatenate([rng.uniform(-0.5, 0.5, (nd, d)), rng.uniform(0.0, 0.5, (nd, 1))], axis=1).astype(np.float16).astype(np.float32)
bdy = np.concatenate([rng.uniform(-0.5, 0.5, (nb, d)), rng.uniform(0.0, 0.5, (nb, 1))], axis=1).astype(np.float16).astype(np.float32)
bdy[np.arange(nb), rng.integers(0, d, nb)] = 0.5
result = {"d": d, "n_domain": nd, "n_boundary": nb, "M": 4 * nd + nb, "reps": reps, "fp64_mfma_peak_tflops": PEAK_TFLOPS, "device": torch.cuda.get_device_name(0),
          "covariance": {}, "sampling": {}}
points = {n: torch.from_numpy(rng.uniform(-0.5, 0.5, (n, d + 1)).astype(np.float32)).cuda() for n in (1200, 4096)}
s = _lib.stream_ptr()
for compat in (None, "reference"):
    gp = GP_Grad_Dependent_Nonlinear(Grad_Dependent_Nonlinear(d + 1), compat=compat)
    gp.kernel_phi_phi(dom, bdy)
    L = gp._L_pad
    Mp = L.shape[0]
    as_coded = compat == "reference"
    idx = gp.laplacian_idx.ctypes.data_as(C.c_void_p) if as_coded else None
    r16 = gp._gram_bits(gp._xd, gp._xb, False) if as_coded else 0
    for n, X in points.items():
        rows = torch.zeros((n, Mp), dtype=torch.float64, device="cuda")
        var = torch.empty(n, dtype=torch.float64, device="cuda")
        cov, final = [None], [None]

        def make_rows():
            _lib.check(lib.scasml_gp_cross_rows(d, gp.a, _lib.ptr(gp._xd), nd, _lib.ptr(gp._xb), nb, idx, r16, 0 if as_coded else 1, 0, _lib.ptr(X), n, d + 1,
                                                _lib.ptr(rows), Mp, s), "gp_cross_rows")

        def solve():
            _lib.check(lib.scasml_gp_variance(_lib.ptr(L), Mp, _lib.ptr(rows), Mp, n, 1.0, _lib.ptr(var), s), "gp_variance")

        def prior():
            cov[0] = gp._prior_block(X, X, False)

        def product():
            _lib.check(lib.scasml_gemm_nt_sub(_lib.ptr(cov[0]), n, n, n, _lib.ptr(rows), Mp, _lib.ptr(rows), Mp, Mp, 0, 1, 0, s), "gemm_nt_sub")

        def mirror():
            final[0] = torch.tril(cov[0]) + torch.tril(cov[0], -1).t()

        case = run({"rows": make_rows, "solve": solve, "prior": prior, "product": product, "mirror": mirror})
        case["whole_call"] = run({"predict_covariance": lambda: gp.predict_covariance(X)})["predict_covariance"]
        same = bool(torch.equal(final[0], gp.predict_covariance(X)))
        case["parts_reproduce_the_call_bit_for_bit"] = same
        case["sum_of_parts_ms"] = sum(case[k]["best_ms"] for k in ("rows", "solve", "prior", "product", "mirror"))
        # flop the lower-only product executes: row r meets the columns of its own 256-row block and of those before it
        executed = 2.0 * Mp * float(sum(min(n, (r // 256 + 1) * 256) for r in range(n)))
        case["product_flop_executed"] = executed
        case["product_tflops_executed"] = executed / case["product"]["best_ms"] / 1e9
        # a sub-selection computed on its own (64 x 64 register-staged tile) against the same entries of the whole call (n = 4096: the 128 x 128
        # LDS-DMA tile) -- the two tile bodies must sum alike for predict_covariance's bit-for-bit claim to hold across that dispatch
        pick = torch.from_numpy(np.sort(np.random.default_rng(n).permutation(n)[:300])).cuda()
        case["sub_selection_of_300_points_same_bits"] = bool(torch.equal(gp.predict_covariance(X[pick]), final[0][pick][:, pick]))
        result["covariance"]["%s n=%d" % (compat or "documented", n)] = case
        print("covariance %-10s n=%4d  rows %.2f | solve %.2f | prior %.2f | product %.2f | mirror %.2f ms | sum %.2f, predict_covariance %.2f ms | product %.1f TFLOP/s executed | same bits %s, sub-selection same bits %s" % (
            compat or "documented", n, case["rows"]["best_ms"], case["solve"]["best_ms"], case["prior"]["best_ms"], case["product"]["best_ms"],
            case["mirror"]["best_ms"], case["sum_of_parts_ms"], case["whole_call"]["best_ms"], case["product_tflops_executed"], same,
            case["sub_selection_of_300_points_same_bits"]), flush=True)
        if as_coded:
            continue
        # ---- sampling: the factor of this covariance + nugget I
        npad = (n + 31) // 32 * 32
        Lc = torch.eye(npad, dtype=torch.float64, device="cuda")
        Lc[:n, :n] = final[0]
        info = torch.zeros(1, dtype=torch.int32, device="cuda")
        _lib.check(lib.scasml_cholesky(_lib.ptr(Lc), npad, float(gp.nugget), _lib.ptr(info), s), "cholesky")
        assert int(info.item()) == 0
        mean = torch.from_numpy(rng.normal(size=n)).cuda()
        for S in (64, 4096):
            out = torch.empty((S, n), dtype=torch.float64, device="cuda")
            comp = torch.empty((S, n), dtype=torch.float64, device="cuda")
            Z = [None]

            def fused():
                _lib.check(lib.scasml_gp_sample(_lib.ptr(Lc), npad, n, _lib.ptr(mean), 7, 0, S, _lib.ptr(out), n, s), "gp_sample")

            def randn():
                Z[0] = torch.randn((S, npad), dtype=torch.float64, device="cuda").neg_()     # C -= A B^T: A = -Z

            def fill():
                comp.copy_(mean[None, :].expand(S, n))

            def gemm():
                _lib.check(lib.scasml_gemm_nt_sub(_lib.ptr(comp), n, S, n, _lib.ptr(Z[0]), npad, _lib.ptr(Lc), npad, npad, 0, 0, 0, s), "gemm_nt_sub")

            case = run({"sample_kernel": fused, "composed_randn": randn, "composed_fill": fill, "composed_gemm_nt_sub": gemm})
            case["composed_route_ms"] = sum(case[k]["best_ms"] for k in ("composed_randn", "composed_fill", "composed_gemm_nt_sub"))
            case["flop_lower_triangle"] = float(S) * n * n
            case["sample_kernel_tflops"] = case["flop_lower_triangle"] / case["sample_kernel"]["best_ms"] / 1e9
            case["sample_kernel_fraction_of_fp64_mfma_peak"] = case["sample_kernel_tflops"] / PEAK_TFLOPS
            case["normal_buffer_bytes_of_the_composed_route"] = 8 * S * npad
            # the composed route's draws are torch's, not the Philox stream's: compare moments only (mean of the draws' means)
            case["mean_of_draw_means_fused_minus_composed"] = float((out.mean(0) - comp.mean(0)).abs().max())
            result["sampling"]["n=%d S=%d" % (n, S)] = case
            print("sampling n=%4d S=%4d  kernel %.3f ms = %.2f TFLOP/s = %.3f of peak | composed: randn %.3f + fill %.3f + gemm_nt_sub %.3f = %.3f ms" % (
                n, S, case["sample_kernel"]["best_ms"], case["sample_kernel_tflops"], case["sample_kernel_fraction_of_fp64_mfma_peak"],
                case["composed_randn"]["best_ms"], case["composed_fill"]["best_ms"], case["composed_gemm_nt_sub"]["best_ms"], case["composed_route_ms"]), flush=True)
with open(out_path, "w") as f:
    json.dump(result, f, indent=1, sort_keys=True)
    f.write("\n")
