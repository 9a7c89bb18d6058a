#!/usr/bin/env python
"""Accuracy and time of the GP leave-one-out kernels (csrc/gp_loo.hip).
    python tools/gp_loo_bench.py [out.json]        (default profiles/gp_loo_accuracy.json)

Accuracy, at the shapes of tests/test_gpu_gp_loo.py and with its NumPy statement: the largest |device - reference| / unit over the entries of
scasml_gp_gram_da_rows and over q_i, v_i of scasml_gp_loo_da fed NumPy's A = inv(K_p) and alpha (the test asserts 16 times the largest), and the
relative errors of GP.loo_log_predictive's value and gradient against the cap 256 cond(K_p) 2^-53.
Time, at the reference's M = 4200 (d = 20, 1000 + 200 points), both routes in this one process, back to back: one scasml_gp_loo_da call against
the composed route the rows kernel makes possible -- the full K_a by scasml_gp_gram_da_rows, T = -A K_a^T by scasml_gemm_nt_sub into a zeroed
Mp x Mp buffer, the row-dot with A in torch.  HIP events around one call, 3 warm-up calls, 20 timed, median and best."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import torch

import _gp_loo_ref as ref
import test_gpu_gp_loo as t
from scasml_gp_amd import _lib

out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "gp_loo_accuracy.json")
lib = _lib.load()
doc = {"device": torch.cuda.get_device_name(0),
       "unit": "gram_da_rows: |device - longdouble K_a from exact differences| / (2^-53 (|P_a| + r^2 |P| / 2) kappa + |d entry / d r^2| (d + 1) 2^-53 "
               "(|x|^2 + |y|^2)); loo_da: |device - longdouble sum| / (2^-53 * sum |terms| of the row), NumPy's A = inv(K_p) and alpha as inputs; "
               "class: |device - NumPy| / sum |terms| of GP.loo_log_predictive, the device solving with K_p itself",
       "shapes": {}}
for (d, nd, nb) in ref.SHAPES:
    rr = t.gram_da_rows_ratio(d, nd, nb)
    rq, rv, cap_ratio = t.loo_da_ratios(d, nd, nb)
    c = t._case(d, nd, nb)
    value, terms, grads, cond = ref.loo_and_grad(d, c["dom"], c["bdy"], c["sigma"], t.NUGGET, c["z"])
    gp = t._gp(d)
    gp.kernel_phi_phi(c["dom"], c["bdy"])
    v, grad = gp.loo_log_predictive(c["z"], return_grad=True)
    key = "d=%d n_dom=%d n_bdy=%d" % (d, nd, nb)
    doc["shapes"][key] = {
        "gram_da_rows": rr, "q": rq, "v": rv, "cap_as_ratio_256_cond": cap_ratio, "a_priori_2_Mp": 2 * ((c["M"] + 31) // 32 * 32), "cond_Kp": cond,
        "cap": ref.cap(cond), "class_value": abs(v - value) / float(np.abs(terms).sum()),
        "class_dlog_sigma": abs(grad["log_sigma"] - float(sum(grads["log_sigma"]).sum())) / float(sum(np.abs(x).sum() for x in grads["log_sigma"])),
        "class_dlog_nugget": abs(grad["log_nugget"] - float(sum(grads["log_nugget"]).sum())) / float(sum(np.abs(x).sum() for x in grads["log_nugget"]))}
    print(key, doc["shapes"][key], flush=True)
doc["largest_gram_da_rows_ratio"] = max(v["gram_da_rows"] for v in doc["shapes"].values())
doc["largest_loo_da_ratio"] = max(max(v["q"], v["v"]) for v in doc["shapes"].values())

d, nd, nb = 20, 1000, 200
dom, bdy = ref.points(d, nd, nb)
gp = t._gp(d)
gp.kernel_phi_phi(dom, bdy)
M, Mp = gp.phi_dim, gp._L_pad.shape[0]
s = _lib.stream_ptr()
A = torch.empty((Mp, Mp), dtype=torch.float64, device="cuda")
_lib.check(lib.scasml_cholesky_inverse(_lib.ptr(gp._L_pad), Mp, _lib.ptr(A), s), "cholesky_inverse")
alpha = torch.randn(M, dtype=torch.float64, device="cuda", generator=torch.Generator(device="cuda").manual_seed(0))
a = gp.a
q, v = (torch.empty(M, dtype=torch.float64, device="cuda") for _ in range(2))
work = torch.empty(int(lib.scasml_gp_loo_da_doubles(nd, nb, 0)), dtype=torch.float64, device="cuda")
Ka = torch.zeros((Mp, Mp), dtype=torch.float64, device="cuda")          # the composed route's two Mp x Mp temporaries
T = torch.empty((Mp, Mp), dtype=torch.float64, device="cuda")


def fused():
    _lib.check(lib.scasml_gp_loo_da(d, a, _lib.ptr(gp._xd), nd, _lib.ptr(gp._xb), nb, _lib.ptr(A), Mp, _lib.ptr(alpha), 0, _lib.ptr(q), _lib.ptr(v),
                                    _lib.ptr(work), s), "gp_loo_da")


def composed():
    _lib.check(lib.scasml_gp_gram_da_rows(d, a, _lib.ptr(gp._xd), nd, _lib.ptr(gp._xb), nb, 0, M, M, _lib.ptr(Ka), Mp, s), "gp_gram_da_rows")
    T.zero_()
    _lib.check(lib.scasml_gemm_nt_sub(_lib.ptr(T), Mp, Mp, Mp, _lib.ptr(A), Mp, _lib.ptr(Ka), Mp, Mp, 0, 0, 0, s), "gemm_nt_sub")      # T = -A K_a^T
    return -(T[:M, :M] * A[:M, :M]).sum(1), Ka[:M, :M] @ alpha


def time_ms(fn, reps=20):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    ts = []
    for _ in range(reps):
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        ts.append(e0.elapsed_time(e1))
    return {"median_ms": float(np.median(ts)), "best_ms": float(min(ts))}


qc, vc = composed()
fused()
flop = 2.0 * M * Mp * Mp
tf, tc = time_ms(fused), time_ms(composed)
doc["timing_M4200"] = {"shape": {"d": d, "n_dom": nd, "n_bdy": nb, "M": M, "Mp": Mp}, "gp_loo_da": tf, "composed_rows_gemm_nt_sub_torch_row_dot": tc,
                       "flop_2_M_Mp2": flop, "gp_loo_da_tflops": flop / (tf["median_ms"] * 1e9),
                       "fused_workspace_doubles": int(work.numel()), "composed_temporaries_doubles": 2 * Mp * Mp,
                       "largest_gap_q_fused_vs_composed_relative": float(((q - qc).abs().max() / qc.abs().max()).item()),
                       "largest_gap_v_fused_vs_composed_relative": float(((v - vc).abs().max() / vc.abs().max()).item()),
                       "method": "HIP events around one call, 3 warm-up calls, 20 timed, both routes in one process back to back; composed: the full K_a "
                                 "by scasml_gp_gram_da_rows, T = -A K_a^T by scasml_gemm_nt_sub into a zeroed Mp x Mp buffer, -(T * A).sum(1) in torch"}
print(doc["timing_M4200"], flush=True)
with open(out_path, "w") as f:
    json.dump(doc, f, indent=1, sort_keys=True)
    f.write("\n")
