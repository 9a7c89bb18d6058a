#!/usr/bin/env python
"""Accuracy and time of the GP evidence kernels (csrc/gp_evidence.hip).
    python tools/gp_evidence_bench.py [out.json]        (default profiles/gp_evidence_accuracy.json)

Accuracy, at the shapes of tests/test_gpu_gp_evidence.py and with its NumPy statement: |device - NumPy| / (2^-53 sum |terms|) of
scasml_gp_gram_da_contract and scasml_chol_logdet fed NumPy's A = inv(K_p), alpha and factor (the test asserts 16 times the largest), and the
relative errors of GP.log_marginal_likelihood's value and gradient against the cap 256 cond(K_p) 2^-53.
Time, at the reference's M = 4200 (d = 20, 1000 + 200 points): one scasml_gp_gram_da_contract call against materialising K_a -- as the central
difference (K(a + h) - K(a - h)) / 2h of two scasml_gp_gram launches, the library has no kernel that stores K_a -- and contracting it with two
torch reductions.  HIP events around one call, 3 warm-up calls, 20 timed, median and best."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import torch

import _gp_evidence_ref as ref
import test_gpu_gp_evidence as t
from scasml_gp_amd import _lib

out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "gp_evidence_accuracy.json")
lib = _lib.load()
doc = {"device": torch.cuda.get_device_name(0),
       "unit": "kernels: |device - NumPy| / (2^-53 * sum |terms|), NumPy's A = inv(K_p), alpha and Cholesky factor as inputs; "
               "class: |device - NumPy| / sum |terms| of GP.log_marginal_likelihood, the device solving with K_p itself",
       "shapes": {}}
for (d, nd, nb) in ref.SHAPES:
    rq, rt, cap_ratio = t.contraction_ratios(d, nd, nb)
    rl, _ = t.logdet_ratio(d, nd, nb)
    c = t._case(d, nd, nb)
    _, _, grads, cond = ref.lml_and_grad(d, c["dom"], c["bdy"], c["sigma"], t.NUGGET, c["z"])
    gp = t._gp(d)
    gp.kernel_phi_phi(c["dom"], c["bdy"])
    value, grad = gp.log_marginal_likelihood(c["z"], return_grad=True)
    doc["shapes"]["d=%d n_dom=%d n_bdy=%d" % (d, nd, nb)] = {
        "alpha_Ka_alpha": rq, "A_Ka": rt, "logdet": rl, "cap_as_ratio_256_cond": cap_ratio, "cond_Kp": cond, "cap": ref.cap(cond),
        "class_value": abs(value - c["value"]) / sum(abs(x) for x in c["terms"]),
        "class_dlog_sigma": abs(grad["log_sigma"] - sum(grads["log_sigma"])) / sum(abs(x) for x in grads["log_sigma"]),
        "class_dlog_nugget": abs(grad["log_nugget"] - sum(grads["log_nugget"])) / sum(abs(x) for x in grads["log_nugget"])}
    print(d, nd, nb, doc["shapes"]["d=%d n_dom=%d n_bdy=%d" % (d, nd, nb)], flush=True)
doc["largest_contraction_ratio"] = max(max(v["alpha_Ka_alpha"], v["A_Ka"]) for v in doc["shapes"].values())
doc["largest_logdet_ratio"] = max(v["logdet"] for v in doc["shapes"].values())

d, nd, nb = 20, 1000, 200
dom, bdy = ref.points(d, nd, nb)
gp = t._gp(d)
gp.kernel_phi_phi(dom, bdy)
M, Mp = gp.phi_dim, gp._L_pad.shape[0]
s = _lib.stream_ptr()
A = torch.empty((Mp, Mp), dtype=torch.float64, device="cuda")
_lib.check(lib.scasml_cholesky_inverse(_lib.ptr(gp._L_pad), Mp, _lib.ptr(A), s), "cholesky_inverse")
alpha = torch.randn(M, dtype=torch.float64, device="cuda", generator=torch.Generator(device="cuda").manual_seed(0))
work = torch.empty(int(lib.scasml_gp_gram_da_contract_doubles(nd, nb)), dtype=torch.float64, device="cuda")
a, h = gp.a, 1e-5 * gp.a
K1 = torch.empty((M, M), dtype=torch.float64, device="cuda")
K2 = torch.empty((M, M), dtype=torch.float64, device="cuda")


def contract():
    _lib.check(lib.scasml_gp_gram_da_contract(d, a, _lib.ptr(gp._xd), nd, _lib.ptr(gp._xb), nb, _lib.ptr(A), Mp, _lib.ptr(alpha), _lib.ptr(work), s),
               "gp_gram_da_contract")


def materialise():
    _lib.check(lib.scasml_gp_gram(d, a + h, _lib.ptr(gp._xd), nd, _lib.ptr(gp._xb), nb, _lib.ptr(K1), s), "gp_gram")
    _lib.check(lib.scasml_gp_gram(d, a - h, _lib.ptr(gp._xd), nd, _lib.ptr(gp._xb), nb, _lib.ptr(K2), s), "gp_gram")
    Ka = (K1 - K2).div_(2 * h)
    return torch.dot(alpha, Ka @ alpha), (A[:M, :M] * Ka).sum()


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


q, tr = materialise()
contract()
doc["timing_M4200"] = {"shape": {"d": d, "n_dom": nd, "n_bdy": nb, "M": M, "Mp": Mp}, "gp_gram_da_contract": time_ms(contract),
                       "materialise_central_difference_and_two_torch_reductions": time_ms(materialise),
                       "contract_values": work[:2].tolist(), "central_difference_values": [float(q), float(tr)],
                       "method": "HIP events around one call, 3 warm-up calls, 20 timed; the comparator builds K_a as (K(a+h) - K(a-h)) / 2h, h = 1e-5 a, "
                                 "from two scasml_gp_gram launches, then alpha . (K_a alpha) and (A * K_a).sum() in torch"}
print(doc["timing_M4200"], flush=True)
with open(out_path, "w") as f:
    json.dump(doc, f, indent=1, sort_keys=True)
    f.write("\n")
