"""The column map of the as-coded matrix-core evaluation (csrc/gp_eval_compat_mfma.hip, compat_tail_packed) at every edge of its rule.

K-steps 0 .. KS-2 hold the first 16 (KS - 1) columns of a point; the last K-step holds the r = max(0, d + 1 - 16 (KS - 1)) that are left and
the three constant columns.  Where 2 r + 4 <= 16 the low parts of the tail share the last step's one MFMA with the high parts (two-plane
forms; with one plane only the map moves).  The shapes are the smallest at which that map can go wrong:

    d = 5    KS = 1, packed, r = 6: all sixteen slots used        d = 6    KS = 1, the first unpacked
    d = 14   KS = 2, r = 0 (the last column alone is padding)     d = 15   KS = 2, r = 0 (first K-step full)
    d = 21   KS = 2, r = 6: the last packed tail                  d = 22   KS = 2, the first unpacked
    d = 100  KS = 7, r = 5: the headline

each with 40 domain + 24 boundary collocation points (a domain tile and a tile of domain and boundary rows) and with 40 + 30 (a third tile of
boundary and padding rows), and 96 evaluation points = three 32-row sites of kinds 0, 4, 3, evaluated in one workgroup in the full form and site
by site, each in the form of its kind.  Reference: the float64 kernel (scasml_gp_eval_compat).  Bounds: tests/test_gpu_compat_mfma.py's, as they
stand -- 2e-5 of sum |c P| per operator row, plus a few float16 ulps of the largest terms where entries are rounded, plus the one-plane term.

Negative control (d = 21, d = 100): one coordinate of the tail moved by 2^-13 of itself -- less than the half ulp 2^-12 of its float16 high
part, so a kernel whose relocated low parts were dead would see the same point (or, across a rounding boundary, one moved by 2^-11) and miss
the float64 kernel's move by about its whole size, ratio ~1.  A live low part leaves float32 noise: the exponent carries ~(d + 4) 2^-24 of
sum |terms| ~ 5, i.e. <= 2e-6 absolute, against a move of a |x_k| |x_k - y_k| 2^-13 >= 6e-5 in the exponent at |x_k| >= 1.5 (a = 16 / d):
ratio <= 0.05.  Asserted: 0.25, between the two in the ratio's logarithm.
"""
import ctypes as C
import functools

import numpy as np
import pytest

from test_gpu_compat_mfma import _magnitudes, _raw, _setup, _test_points

pytestmark = pytest.mark.gpu

SHAPES = [5, 6, 14, 15, 21, 22, 100]
PACKED = {5: True, 6: False, 14: True, 15: True, 21: True, 22: False, 100: True}
COLLOC = [(40, 24), (40, 30)]
KINDS = [0, 4, 3]
CASES = [(d, nd, nb) for d in SHAPES for nd, nb in COLLOC]
IDS = ["d%d-%d+%d" % c for c in CASES]
GEOMETRY_CASES = [c for c in CASES if c[0] in (21, 100)]


def _hutch(d):
    """Five distinct Hutchinson indices with 0 and d - 1 among them: the tail feeds the Laplacian too."""
    return [d - 1, 0, d // 2, 1, d - 2]


def _float64_kernel(gp, X, round16):
    """(out4, lap) of scasml_gp_eval_compat: the float64 statement on the device (csrc/gp_compat.hip)."""
    import torch
    from scasml_gp_amd import _lib
    lib = _lib.load()
    pts = gp._points_device(X)[0]
    out4 = torch.zeros((pts.shape[0], 4), dtype=torch.float32, device="cuda")
    lap = torch.zeros((pts.shape[0],), dtype=torch.float32, device="cuda")
    _lib.check(lib.scasml_gp_eval_compat(
        gp.d, gp.a, float(gp.equation.sigma()), float(gp.equation.mu()), int(gp.equation.eq_id), *gp._f64_model(), round16, _lib.ptr(pts), pts.shape[0],
        pts.shape[1], _lib.ptr(out4), _lib.ptr(lap), _lib.stream_ptr()), "gp_eval_compat")
    return out4.cpu().numpy().astype(np.float64), lap.cpu().numpy().astype(np.float64)


def _one_site(gp, X, round16, site):
    """out4 of a launch over one listed 32-row site: its workgroup runs the form of that site's kind."""
    import torch
    from scasml_gp_amd import _lib
    lib = _lib.load()
    pts = gp._points_device(X)[0]
    kd = torch.from_numpy(np.asarray(KINDS, dtype=np.uint8)).cuda()
    od = torch.from_numpy(np.asarray([site], dtype=np.int32)).cuda()
    out4 = torch.full((pts.shape[0], 4), -7.0, dtype=torch.float32, device="cuda")
    _lib.check(lib.scasml_gp_eval_compat_site_list(
        gp.d, gp.a, float(gp.equation.sigma()), float(gp.equation.mu()), int(gp.equation.eq_id), _lib.ptr(gp._compat_model), gp.N_domain, gp.N_boundary,
        gp.laplacian_idx.ctypes.data_as(C.c_void_p), round16, 0.0, _lib.ptr(pts), pts.shape[0], 32, _lib.ptr(kd), _lib.ptr(od), 1, _lib.ptr(out4), None,
        _lib.stream_ptr()), "gp_eval_compat_site_list")
    got = out4.cpu().numpy().astype(np.float64)
    others = np.ones(len(X), dtype=bool)
    others[site * 32:(site + 1) * 32] = False
    assert (got[others] == -7.0).all()
    return got[site * 32:(site + 1) * 32]


@functools.lru_cache(maxsize=None)
def _case(d, nd, nb):
    """One fit, one set of points and the float64 kernel's answers (entries rounded and not), shared by the tests of a shape."""
    gp, ogp, _ = _setup(d, _hutch(d), nd, nb, seed=100 + d)
    X = _test_points(d, 32 * len(KINDS), seed=200 + d)
    ref = {}
    for rounded in (False, True):
        ogp.round16, ogp.round_out = rounded, False
        mag = _magnitudes(ogp, X)
        # a rounding decided on float32 here and on float64 there moves one term by 2^-11 of itself: a few of the largest per point
        flip = {op: (4 * 2.0 ** -11 * (np.abs(ogp._features(op, X)) * np.abs(ogp.right_vector)[:, 0][None, :]).max(1)) if rounded else 0.0 for op in mag}
        ref[rounded] = (_float64_kernel(gp, X, 1 if rounded else 0), mag, flip)
    ycol = np.concatenate([ogp.x_t_domain, ogp.x_t_boundary])
    loose = gp.a * 2.0 ** -12 * float((np.abs(X).astype(np.float64) @ np.abs(ycol).T).max())     # one point plane (tests/test_gpu_compat_mfma.py)
    return gp, X, ref, loose


def _check(tag, got4, got_lap, want4, want_lap, mag, flip, tol, rows=slice(None), cols=("I", "div", "dt", "lap")):
    col = {"I": 0, "div": 1, "dt": 3}
    worst = {}
    for op in cols:
        err = np.abs((got_lap - want_lap) if op == "lap" else (got4[:, col[op]] - want4[rows, col[op]]))
        bound = tol * mag[op][rows] + (flip[op][rows] if isinstance(flip[op], np.ndarray) else 0.0)
        worst[op] = float((err / bound).max())
    print("%s: largest error / bound %s" % (tag, {k: round(v, 4) for k, v in worst.items()}))
    assert all(v <= 1.0 for v in worst.values()), (tag, worst)


def test_the_shapes_sit_on_both_sides_of_the_packing_rule():
    from scasml_gp_amd import _lib
    lib = _lib.load()
    for d in SHAPES:
        kp = int(lib.scasml_point_stride(d))
        r = max(0, d + 1 - (kp - 16))
        assert (2 * r + 4 <= 16) == PACKED[d], (d, kp, r)
    assert [int(lib.scasml_point_stride(d)) // 16 for d in SHAPES] == [1, 1, 2, 2, 2, 2, 7]


@pytest.mark.parametrize("d,nd,nb", CASES, ids=IDS)
def test_as_coded_form_matches_the_float64_kernel(d, nd, nb):
    gp, X, ref, _ = _case(d, nd, nb)
    (want4, want_lap), mag, flip = ref[True]
    out1, lap1 = _raw(gp, X, round16=1)                    # entries rounded, outputs not: the sums themselves
    _check("d=%d as coded, full form" % d, out1, lap1, want4, want_lap, mag, flip, 2e-5)
    out3, lap3 = _raw(gp, X, round16=3)                    # as the solvers call it: u_hat and eps_PDE leave as float16 values
    assert np.array_equal(out3[:, 0].astype(np.float16).astype(np.float64), out3[:, 0])
    assert np.array_equal(out3[:, 2].astype(np.float16).astype(np.float64), out3[:, 2])
    assert np.all(np.abs(out3[:, 0] - out1[:, 0]) <= 2.0 ** -11 * np.abs(out1[:, 0]) + 1e-7)
    assert np.array_equal(out3[:, [1, 3]], out1[:, [1, 3]]) and np.array_equal(lap3, lap1)
    # each site in the form of its kind: what it consumes has the full form's bits
    for s, k in enumerate(KINDS):
        part = _one_site(gp, X, 3, s)
        full = out3[s * 32:(s + 1) * 32]
        assert np.array_equal(part[:, 0], full[:, 0]), (s, k)
        if k in (0, 4):
            assert np.array_equal(part[:, 1], full[:, 1]), (s, k)
        if k == 0:
            assert np.array_equal(part, full), (s, k)


@pytest.mark.parametrize("d,nd,nb", GEOMETRY_CASES, ids=["d%d-%d+%d" % c for c in GEOMETRY_CASES])
@pytest.mark.parametrize("bits", [0, 4], ids=["two-planes", "one-plane"])
def test_geometry_mode_matches_the_float64_kernel(bits, d, nd, nb):
    gp, X, ref, loose = _case(d, nd, nb)
    (want4, want_lap), mag, flip = ref[False]
    tol = 2e-5 + (loose if bits else 0.0)
    out, lap = _raw(gp, X, round16=bits)
    _check("d=%d geometry bits=%d, full form" % (d, bits), out, lap, want4, want_lap, mag, flip, tol)
    for s, k in enumerate(KINDS):
        rows = slice(s * 32, (s + 1) * 32)
        part = _one_site(gp, X, bits, s)
        _check("d=%d geometry bits=%d, site kind %d" % (d, bits, k), part, None, want4, None, mag, flip, tol, rows,
               {0: ("I", "div", "dt"), 4: ("I", "div"), 3: ("I",)}[k])


@pytest.mark.parametrize("d,nd,nb", [c for c in CASES if c[0] in (21, 100) and c[2] == 24], ids=["d21", "d100"])
def test_the_low_parts_of_the_packed_tail_are_live(d, nd, nb):
    gp, X, _, _ = _case(d, nd, nb)
    k = 16 * ((d + 4 + 15) // 16 - 1) + 2                  # a coordinate of the last K-step's tail: x_18 of 16 .. 21, x_98 of 96 .. 100
    assert 16 * ((d + 4 + 15) // 16 - 1) <= k < d
    rng = np.random.default_rng(d)
    X0 = X.copy()
    X0[:, k] = rng.uniform(1.5, 1.9, len(X)).astype(np.float32) * rng.choice([-1.0, 1.0], len(X)).astype(np.float32)
    X1 = X0.copy()
    X1[:, k] = X0[:, k] * np.float32(1.0 + 2.0 ** -13)
    assert np.all(X1[:, k] != X0[:, k]) and np.abs(X1).max() < 2.0
    want = _float64_kernel(gp, X1, 0)[0] - _float64_kernel(gp, X0, 0)[0]
    got = _raw(gp, X1, round16=0)[0] - _raw(gp, X0, round16=0)[0]          # smooth form, both point planes
    for name, c in (("u_hat", 0), ("div", 1), ("dt", 3)):
        ratio = float(np.linalg.norm(got[:, c] - want[:, c]) / np.linalg.norm(want[:, c]))
        print("d=%d %s: |move - float64 move| / |float64 move| = %.4f (move %.3e)" % (d, name, ratio, np.linalg.norm(want[:, c])))
        assert ratio <= 0.25, (name, ratio)
