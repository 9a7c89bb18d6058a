"""The Picard passes' arithmetic changes that must not move a result (csrc/picard_tree.hpp): the sum over dims taken in registers (group_sum:
DPP operands and one swizzle -- the same butterfly, the same partners) and ACCUMULATE's level-0 nodes without their "+" addend (an exact
zero).  GENERATE's rows are held too: its lane mapping was tried over the quads that hold a spatial dim, and any further try has to write the
same bytes.

Every case is compared with what the library of the commit BEFORE these changes returned on an MI355X for the same inputs
(tests/golden/picard_dim_sum_parent.npz, written by tests/golden/make_picard_dim_sum.py):

* out_uz, out_uhat and the standard errors equal BY VALUE (np.array_equal, a NaN equal to a NaN).  Not by bit pattern: v - v = +0, u + 0 = u and fma(0, W, z) = z
  leave every value, but the sign of a zero that the dropped addend used to decide may differ;
* GENERATE's point buffer, filled with 7.0 before the launch on both sides, by the SHA-256 of its bytes: a column of the tail that stops being
  written, a moved t, a changed normal or a row of another rank that gets written all change the hash.

Shapes: B = 5 roots (a partly filled last wave at every G; four ordinary roots and one 2^-10 below T, where ACCUMULATE replays its normals
instead of reading them back); d = 3, 4, 12 | 13, 28 | 29, 30, 60 | 61, 100, 124 | 125, 252 (G = 4, 8, 16, 32, 64 at both ends of their ranges; d
mod 4 = 0, 1, 2, 3; d = 4, 12, 28, 60, 100, 124, 252: t in a float4 of its own; d = 3, 4: one live quad and three more float4 in the row); n = rho = 1, 2, 3 in quadrature, n = 1 with rho = 2 beside them (at rho = 1 the
reference's one-node rule has the weight 0 / 0: every output is NaN before and after, and NaN must stay where it was), and n = 2, M = 2 in full
history; MLP mode
(equation 0), GENERATE -> ACCUMULATE; both with standard errors at d = 100, n = 2 (rho = 3: a term of one sample has no estimate); the
reference's stream at d = 20, n = 2; ACCUMULATE sample-sharded over two ranks at d = 100, n = 2.

Inputs are exact everywhere (integer hashes scaled by powers of two, no library function): the roots, and the surrogate's values in `vals`,
which stand in for the GP evaluation (u_hat near g's range, div, eps_PDE, d_t).  The clip is 1e6 so that no result hides behind it.
"""
import ctypes as C
import functools
import hashlib
import os
import sys

import numpy as np
import pytest

for _p in (os.path.dirname(os.path.abspath(__file__)), os.path.dirname(os.path.dirname(os.path.abspath(__file__)))):      # imported by the recorder too
    if _p not in sys.path:
        sys.path.insert(0, _p)
from test_gpu_picard_sweep import _G, _Tree

gpu = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "picard_dim_sum_parent.npz")
B = 5
DIMS = [3, 4, 12, 13, 28, 29, 30, 60, 61, 100, 124, 125, 252]
PLANS = [("quad", 1, 1), ("quad", 1, 2), ("quad", 2, 2), ("quad", 3, 3), ("fh", 2, 2)]
NAN_PLAN = ("quad", 1, 1)         # rho = 1: the tabulated weight of its one-node rule is NaN (0 / 0, as in the reference), so every output is NaN
SENTINEL = 7.0
CLIP = 1e6
MLP, ACC = "mlp", "acc"
# (name, d, variant, n, par, mode, extra): extra = "" | "se" | "jax" | "rank0" | "rank1"
CASES = [("%s-d%d-%s%d-%d" % (mode, d, v, n, par), d, v, n, par, mode, "") for d in DIMS for v, n, par in PLANS for mode in (MLP, ACC)]
CASES += [("%s-d100-quad2-se" % mode, 100, "quad", 2, 3, mode, "se") for mode in (MLP, ACC)]
CASES += [("%s-d20-quad2-jax" % mode, 20, "quad", 2, 2, mode, "jax") for mode in (MLP, ACC)]
CASES += [("acc-d100-quad2-rank%d" % r, 100, "quad", 2, 2, ACC, "rank%d" % r) for r in range(2)]


def _hash01(n, salt):
    """n exact multiples of 2^-24 in [0, 1): a 32-bit integer hash of the index (two xorshift-multiply rounds), top 24 bits."""
    x = (np.arange(n, dtype=np.uint64) + np.uint64(1)) * np.uint64(0x9E3779B1) + np.uint64(salt) * np.uint64(0x85EBCA6B)
    for mul in (0x7FEB352D, 0x846CA68B):
        x &= np.uint64(0xFFFFFFFF)
        x ^= x >> np.uint64(15)
        x = x * np.uint64(mul)
    x &= np.uint64(0xFFFFFFFF)
    return (x >> np.uint64(8)).astype(np.float64) * 2.0 ** -24


def _roots(d):
    """x in (-1/2, 1/2) 2^-k with 2^k >= sqrt(d) / 2, so that T + sum x stays where g = 1 - 1 / (1 + exp(.)) has slope; t in [1/16, 5/16), the
    last root 2^-10 below T = 1/2 (sigma sqrt(T - t) = 0.0078, below the read-back switch at 1e-2)."""
    scale = 2.0 ** -int(np.ceil(np.log2(max(d, 4)) / 2 - 1))
    xt = np.empty((B, d + 1), dtype=np.float32)
    xt[:, :d] = ((_hash01(B * d, 11 + d) - 0.5) * scale).reshape(B, d)
    xt[:, d] = 0.0625 + 0.25 * _hash01(B, 13 + d)
    xt[B - 1, d] = np.float32(0.5 - 2.0 ** -10)
    return xt


def _vals(rows, salt):
    """(rows, 4) float32: u_hat in [1/4, 3/4), sum_i d_i u_hat in [-1/4, 1/4), eps_PDE in [-1/32, 1/32), d_t u_hat in [-1/2, 1/2)."""
    h = _hash01(rows * 4, salt).reshape(rows, 4)
    return np.stack([0.25 + 0.5 * h[:, 0], 0.5 * h[:, 1] - 0.25, 0.0625 * h[:, 2] - 0.03125, h[:, 3] - 0.5], axis=1).astype(np.float32)


def run_case(d, variant, n, par, mode, extra):
    """-> dict of float32 arrays (uz; uhat in ACCUMULATE; se with standard errors) and, in ACCUMULATE, the SHA-256 of GENERATE's buffer."""
    import torch
    from scasml_gp_amd import _lib
    lib = _lib.load()
    t = _Tree(0, d, variant, surrogate=mode == ACC)
    prob = _lib.Problem(t.prob.d, t.prob.eq_id, t.prob.T, t.prob.mu, t.prob.sigma, CLIP)
    assert t.prob.T == 0.5
    plan = t.plan(n, par)
    if extra.startswith("rank"):
        rng = t.rng(rank=int(extra[4:]), world=2)
    else:
        rng = t.rng(jax=(n, par) if extra == "jax" else None)
    x = torch.from_numpy(_roots(d)).cuda()
    out = torch.full((B, d + 1), -3.0, dtype=torch.float32, device="cuda")
    res = {}
    pts = vals = uh = None
    if mode == ACC:
        ppr = int(lib.scasml_points_per_root(C.byref(plan)))
        pts = torch.full((ppr * B, t.kp), SENTINEL, dtype=torch.float32, device="cuda")
        _lib.check(t.launch(_lib.MODE_GENERATE, plan, x, B, 0, rng, pts=pts, prob=prob), "picard_tree(generate)")
        res["points_sha256"] = np.array(hashlib.sha256(pts.cpu().numpy().tobytes()).hexdigest())
        vals = torch.from_numpy(_vals(ppr * B, 1000 * n + d)).cuda()
        uh = torch.full((B,), -3.0, dtype=torch.float32, device="cuda")
    kmode = _lib.MODE_ACCUMULATE if mode == ACC else _lib.MODE_MLP
    if extra == "se":
        se = torch.full((B,), -3.0, dtype=torch.float32, device="cuda")
        _lib.check(lib.scasml_picard_tree_stderr(C.byref(prob), C.byref(plan), kmode, _lib.ptr(x), B, 0, rng, _lib.ptr(pts), _lib.ptr(vals),
                                                 _lib.ptr(out), _lib.ptr(uh), _lib.ptr(se), _lib.stream_ptr()), "picard_tree_stderr")
        torch.cuda.synchronize()
        res["se"] = se.cpu().numpy()
    else:
        _lib.check(t.launch(kmode, plan, x, B, 0, rng, pts=pts, vals=vals, out=out, uhat=uh, prob=prob), "picard_tree")
    res["uz"] = out.cpu().numpy()
    if uh is not None:
        res["uhat"] = uh.cpu().numpy()
    return res


def record(path):
    """The fixture: every case's results under '<case>/<key>'.  Refuses results that say nothing: non-finite (but NAN_PLAN's), clipped, mostly zero."""
    out, bad = {}, []
    for name, d, variant, n, par, mode, extra in CASES:
        for key, v in run_case(d, variant, n, par, mode, extra).items():
            if v.dtype == np.float32 and (variant, n, par) == NAN_PLAN and key == "uz":
                if not np.isnan(v).all():
                    bad.append((name, key, "not NaN"))
            elif v.dtype == np.float32 and not (np.isfinite(v).all() and np.abs(v).max() < CLIP and np.count_nonzero(v) > v.size // 2):
                bad.append((name, key, float(np.abs(v).max()), int(np.count_nonzero(v)), v.size))
            out[name + "/" + key] = v
    assert not bad, bad
    np.savez_compressed(path, **out)
    return out


@functools.lru_cache(maxsize=None)
def _golden():
    with np.load(GOLDEN) as z:
        return {k: z[k] for k in z.files}


def test_the_cases_reach_every_width_residue_and_mode():
    assert sorted({_G(d) for d in DIMS}) == [4, 8, 16, 32, 64] and {d % 4 for d in DIMS} == {0, 1, 2, 3}
    for g in (4, 8, 16, 32, 64):                                   # both ends of every G's range but d = 1 (one live quad, nothing to sum)
        ds = [d for d in range(1, 253) if _G(d) == g]
        assert ds[-1] in DIMS and (ds[0] in DIMS or g == 4), g
    assert all((B * _G(d)) % 64 != 0 for d in DIMS if _G(d) < 64) and (B * 64) % 256 != 0      # a partly filled last wave (G = 64: workgroup)
    assert set(PLANS) >= {("quad", 1, 1), ("quad", 2, 2), ("quad", 3, 3)}
    assert {c[6] for c in CASES} == {"", "se", "jax", "rank0", "rank1"}
    want = {c[0] + "/" + k for c in CASES for k in (("uz", "uhat", "points_sha256") if c[5] == ACC else ("uz",)) + (("se",) if c[6] == "se" else ())}
    assert set(_golden()) == want


@gpu
@pytest.mark.parametrize("d", sorted({c[1] for c in CASES}))
def test_results_are_the_parent_commits_by_value(d):
    g = _golden()
    for name, dd, variant, n, par, mode, extra in CASES:
        if dd != d:
            continue
        got = run_case(d, variant, n, par, mode, extra)
        for key, v in got.items():
            want = g[name + "/" + key]
            if key == "points_sha256":
                assert str(v) == str(want), name + ": GENERATE's point buffer"
            else:
                assert v.shape == want.shape and np.array_equal(v, want, equal_nan=True), "%s %s: %d of %d values differ, largest |delta| %g" % (
                    name, key, int(((v != want) & ~(np.isnan(v) & np.isnan(want))).sum()), v.size, float(np.nanmax(np.abs(v.astype(np.float64) - want))))
