"""Every site form of the documented-operator evaluation (scasml_gp_eval_sites, csrc/gp_eval_bf16.hip) at every compiled K-step count and in
every arithmetic mode, against the full form's bits and the float64 statement (oracle/gp.py).

scasml_gp_eval_sites chooses per 32-row wave what the epilogue computes: the full form; u_hat only (form 1, two u-only neighbours may share
it); the folded terminal form (form 2: a kind-3 site, t = T exactly, single-site waves only); u_hat and div (form 3, single-site waves
only); and it returns whole workgroups early that lie inside sites of another rank (kind 2).  The code promises that what a site consumes has
the full form's bits whatever the form -- the folded terminal form alone agrees to rounding only -- and that a point's arithmetic does not
depend on how its batch was cut.  tests/test_gpu_eval_sweep.py sweeps the full form; this module sweeps the rest, with that module's sizes,
collocation counts, modes and bounds:

* layout A, the solvers' (32 rows per site): whole unowned workgroups in front for every workgroup size the launcher uses, then a workgroup
  of every size that begins and ends unowned with owned sites of every kind between (waves of different forms behind the same barriers),
  then every owned kind twice and a partly filled last site whose kind goes round the sweep;
* layout B, 48 rows per site: every ordered pair of kinds as neighbours, and (entered at site 0 and again at site 1) inside one wave;
  forms 2 and 3 must not be taken;
* layout C: kinds that are ignored (fewer than 32 rows per site, no kinds) and refused (no rows per site), and an empty call.

Rows of unowned sites hold NaN in every real column: whatever an owned row gives was computed without them.
"""
import ctypes as C
import functools

import numpy as np
import pytest

from test_gpu_eval_sweep import D_SWEEP, DOC_CASES, DOC_MODES, PREFIXES, _doc_setup, _ks

gpu = pytest.mark.gpu

T_TERMINAL = 0.5            # the equation's terminal time (equations.py: geometry()); the model is packed with it
SENTINEL = -7.0
SCASML_ERR_ARG = -1         # include/scasml_hip.h
WORKGROUP_ROWS = (128, 256, 384, 512)      # 4, 8 or 12 waves of 32 points (gp_eval_bf16.hip, launch_one); 8 waves of 64 (gp_eval.hip)
OWNED = (0, 1, 3, 4)

# ---- layout A
ROWS_A = 32
UNOWNED_ROWS_A = 1536                      # a common multiple of every workgroup size
MIXED_A = [2, 0, 2, 2, 1, 3, 4, 2, 0, 4, 3, 2, 1, 3, 4, 2]            # sites 48..63
TAIL_ROWS = 17


def _kinds_a(d):
    return [2] * (UNOWNED_ROWS_A // ROWS_A) + MIXED_A + [0, 1, 3, 4] * 2 + [OWNED[D_SWEEP.index(d) % 4]]


N_A = 72 * ROWS_A + TAIL_ROWS              # 2321
# ---- layout B: 26 sites whose 25 neighbour pairs are all the ordered pairs of {0, 1, 2, 3, 4}
ROWS_B = 48
KINDS_B = [0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 0, 2, 4, 1, 3, 0, 3, 1, 4, 2, 0, 4, 3, 2, 1, 0]
N_B = 25 * ROWS_B + TAIL_ROWS              # 1217


def _site_slices(kinds, rows, n):
    return [(s, k, slice(s * rows, min((s + 1) * rows, n))) for s, k in enumerate(kinds)]


def _pairs_in_one_wave(kinds, rows):
    return {(kinds[s], kinds[s + 1]) for s in range(len(kinds) - 1) if (s + 1) * rows % 32}


def test_the_layouts_reach_every_form_pair_and_workgroup_cut():
    """The layouts themselves: what the GPU test relies on to reach every form, every pair of forms in one wave and every workgroup cut."""
    pairs = set(zip(KINDS_B, KINDS_B[1:]))
    assert len(KINDS_B) == 26 and pairs == {(i, j) for i in range(5) for j in range(5)}
    assert ROWS_B % 32 and ROWS_B > 32 and (len(KINDS_B) - 1) * ROWS_B + TAIL_ROWS == N_B
    # 48 = 32 + 16: every other site edge lies inside a 32-row wave, so the pairs that share a wave are those at odd edges; the same
    # buffer entered one site later turns the even edges into odd ones, and between them the two launches put every pair into one wave
    in_wave = [_pairs_in_one_wave(KINDS_B[off:], ROWS_B) for off in (0, 1)]
    assert in_wave[0] | in_wave[1] == pairs and len(in_wave[0]) == 13 and len(in_wave[1]) == 12
    assert len(MIXED_A) == 16
    for d in D_SWEEP:
        kinds = _kinds_a(d)
        assert len(kinds) == 73 and (len(kinds) - 1) * ROWS_A + TAIL_ROWS == N_A == 2321
        for wg in WORKGROUP_ROWS:
            assert UNOWNED_ROWS_A % wg == 0 and wg % ROWS_A == 0
            assert all(k == 2 for k in kinds[:UNOWNED_ROWS_A // ROWS_A])                 # rows 0..1535: whole unowned workgroups
            mixed = kinds[UNOWNED_ROWS_A // ROWS_A:(UNOWNED_ROWS_A + wg) // ROWS_A]      # the workgroup that starts at row 1536
            assert mixed[0] == 2 and mixed[-1] == 2 and any(k != 2 for k in mixed[1:-1]), wg
        # the workgroup of 512 rows holds every owned kind, and every owned kind next to an unowned site
        assert set(MIXED_A) == {0, 1, 2, 3, 4}
        assert all(k in kinds[64:72] for k in OWNED)
        assert all(k != 2 for k in kinds[64:])
    # every owned kind as a full site (above) and as a partly filled last one, at both ends of the K-step range
    assert {_kinds_a(d)[-1] for d in D_SWEEP} == set(OWNED)
    assert {_kinds_a(d)[-1] for d in D_SWEEP if _ks(d) <= 2} == set(OWNED) == {_kinds_a(d)[-1] for d in D_SWEEP if _ks(d) >= 15}
    assert 0 < TAIL_ROWS < 32


def _points(d, n, kinds, rows, seed):
    """_doc_setup's recipe (uniform in +-0.6, t = |.|); t = T exactly on kind-3 sites, NaN in every real column on kind-2 sites"""
    X = np.random.default_rng(seed).uniform(-0.6, 0.6, (n, d + 1)).astype(np.float32)
    X[:, -1] = np.abs(X[:, -1])
    for _, k, sl in _site_slices(kinds, rows, n):
        if k == 3:
            X[sl, -1] = T_TERMINAL
        elif k == 2:
            X[sl] = np.nan
    return X


@functools.lru_cache(maxsize=2)
def _sites_setup(d, f16_colloc):
    """The model of tests/test_gpu_eval_sweep.py at (d, f16_colloc), the two point buffers on the device, and the float64 statement with
    its magnitude on layout A's owned rows."""
    gp, ora, _, _, _ = _doc_setup(d, f16_colloc)
    assert float(gp.T) == T_TERMINAL
    kinds_a = _kinds_a(d)
    XA = _points(d, N_A, kinds_a, ROWS_A, seed=d + 11)
    XB = _points(d, N_B, KINDS_B, ROWS_B, seed=d + 12)
    owned = np.concatenate([np.arange(sl.start, sl.stop) for _, k, sl in _site_slices(kinds_a, ROWS_A, N_A) if k != 2])
    Xo = XA[owned]
    assert np.isfinite(Xo).all()
    mag = np.zeros(N_A)
    mag[owned] = (np.abs(ora._features("I", Xo)) @ np.abs(ora.right_vector))[:, 0] + 1e-3
    want = np.full((N_A, 4), np.nan)                      # columns as out4: u, div, eps, dt
    dt, div, _ = ora.pde_parts(Xo)
    want[owned, 0], want[owned, 1] = ora.predict(Xo)[:, 0], div[:, 0]
    want[owned, 2], want[owned, 3] = ora.compute_PDE_loss(Xo)[:, 0], dt[:, 0]
    return gp, ora, kinds_a, XA, gp._points_device(XA)[0], XB, gp._points_device(XB)[0], mag, want


def _model(gp, split, f16_colloc):
    m = gp._device_model()
    m.split = split
    m.x_bound = 0.0
    assert m.split == split and m.colloc_is_f16 == int(f16_colloc)
    return m


def _sites(m, pts, rows, kinds, n=None):
    """out4 of scasml_gp_eval_sites on the first n rows of a device buffer, over a sentinel"""
    import torch
    from scasml_gp_amd import _lib
    lib = _lib.load()
    n = pts.shape[0] if n is None else n
    kd = None if kinds is None else torch.from_numpy(np.asarray(kinds, dtype=np.uint8)).cuda()
    out4 = torch.full((n, 4), SENTINEL, dtype=torch.float32, device="cuda")
    _lib.check(lib.scasml_gp_eval_sites(C.byref(m), _lib.ptr(pts), n, rows, _lib.ptr(kd), _lib.ptr(out4), _lib.stream_ptr()), "gp_eval_sites")
    return out4.cpu().numpy()


def _full(m, pts):
    import torch
    from scasml_gp_amd import _lib
    out4 = torch.full((pts.shape[0], 4), SENTINEL, dtype=torch.float32, device="cuda")
    _lib.check(_lib.load().scasml_gp_eval(C.byref(m), _lib.ptr(pts), pts.shape[0], _lib.ptr(out4), None, _lib.stream_ptr()), "gp_eval")
    return out4.cpu().numpy()


CONSUMED = {0: (0, 1, 2, 3), 1: (0,), 3: (0,), 4: (0, 1)}          # out4 columns a site of each kind consumes


def _same_bits(a, b):
    return np.array_equal(a.view(np.uint32), b.view(np.uint32))


@gpu
@pytest.mark.parametrize("d,mode", DOC_CASES, ids=["ks%02d-d%d-%s" % (_ks(d), d, m) for d, m in DOC_CASES])
def test_site_forms_give_the_full_forms_bits_and_match_the_float64_statement(d, mode):
    from scasml_gp_amd import _lib
    lib = _lib.load()
    split, f16_colloc, tol_u, tol_p = DOC_MODES[mode]
    gp, ora, kinds_a, XA, ptsA, XB, ptsB, mag, want = _sites_setup(d, f16_colloc)
    m = _model(gp, split, f16_colloc)
    tol = np.array([tol_u, tol_p, tol_p, tol_p])[None, :] * np.stack([mag, *[mag * (1 + ora.a * (1 + d))] * 3], axis=1)
    worst = {}

    def note(key, ratio):
        worst[key] = max(worst.get(key, 0.0), float(np.max(ratio)))

    # ---------------------------------------------------------------------------------------- layout A: the solvers'
    full = _full(m, ptsA)
    got = _sites(m, ptsA, ROWS_A, kinds_a)
    if split != 0:                                        # the FP32 kernel evaluates everything
        assert (got[:UNOWNED_ROWS_A] == SENTINEL).all()
    for s, k, sl in _site_slices(kinds_a, ROWS_A, N_A):
        if k == 2:
            continue
        cols = list(CONSUMED[k])
        assert np.isfinite(got[sl][:, cols]).all(), (s, k)
        err = np.abs(got[sl][:, cols].astype(np.float64) - want[sl][:, cols])
        for c in cols:
            note("%s k%d" % ("u div eps dt".split()[c], k), np.abs(got[sl, c] - want[sl, c]) / tol[sl, c])
        assert np.all(err <= tol[sl][:, cols]), (s, k, float(np.max(err / tol[sl][:, cols])))
        if k == 3:                                        # the folded form: to rounding only; both lie within tol_u mag of the statement
            gap = np.abs(got[sl, 0].astype(np.float64) - full[sl, 0])
            note("terminal-full", gap / (2 * tol_u * mag[sl]))
            assert np.all(gap <= 2 * tol_u * mag[sl]), (s, float(np.max(gap / mag[sl])))
        else:
            assert _same_bits(got[sl][:, cols], full[sl][:, cols]), (s, k)
    # a batch cut anywhere gives the same bits: 1, 31 and 33 rows from the first owned site of every kind on, alone, with that
    # site's kinds (33 rows reach one row into the next site: a one-row last site in whatever form its kind selects)
    for k in OWNED:
        s0 = UNOWNED_ROWS_A // ROWS_A + MIXED_A.index(k)
        for n in PREFIXES:
            ks = kinds_a[s0:s0 + -(-n // ROWS_A)]
            part = _sites(m, ptsA[s0 * ROWS_A:], ROWS_A, ks, n)
            for i, ki, sl in _site_slices(ks, ROWS_A, n):
                if ki != 2:
                    cols = list(CONSUMED[ki])
                    whole = got[s0 * ROWS_A + sl.start:s0 * ROWS_A + sl.stop]
                    assert _same_bits(part[sl][:, cols], whole[:, cols]), (k, n, i, ki)

    # ---------------------------------------------------------------------------------------- layout B: straddling waves
    fullB = _full(m, ptsB)
    for off in (0, 1):                                    # entered at site 1 the other half of the site edges lies inside a wave
        kinds, n = KINDS_B[off:], N_B - off * ROWS_B
        gotB = _sites(m, ptsB[off * ROWS_B:], ROWS_B, kinds)
        wantB = fullB if off == 0 else _full(m, ptsB[off * ROWS_B:])
        for s, k, sl in _site_slices(kinds, ROWS_B, n):
            if k != 2:
                cols = list(CONSUMED[k])
                assert np.isfinite(gotB[sl][:, cols]).all(), (off, s, k)
                assert _same_bits(gotB[sl][:, cols], wantB[sl][:, cols]), (off, s, k)

    # ---------------------------------------------------------------------------------------- layout C: kinds ignored and refused
    real = np.isfinite(XB).all(1)
    assert np.isfinite(fullB[real]).all()
    for rows in (16, 1):
        tiled = (KINDS_B * (-(-N_B // (rows * len(KINDS_B))) + 1))[:-(-N_B // rows)]
        assert _same_bits(_sites(m, ptsB, rows, tiled)[real], fullB[real]), rows
    none = _sites(m, ptsB, ROWS_B, None)
    assert _same_bits(none[real], fullB[real]) and np.array_equal(np.isnan(none), np.isnan(fullB))
    import torch
    kd = torch.from_numpy(np.asarray(KINDS_B, dtype=np.uint8)).cuda()
    out4 = torch.full((N_B, 4), SENTINEL, dtype=torch.float32, device="cuda")
    rc = lib.scasml_gp_eval_sites(C.byref(m), _lib.ptr(ptsB), N_B, 0, _lib.ptr(kd), _lib.ptr(out4), _lib.stream_ptr())
    assert rc == SCASML_ERR_ARG and b"rows_per_site" in lib.scasml_last_error()
    assert lib.scasml_gp_eval_sites(C.byref(m), _lib.ptr(ptsB), 0, ROWS_B, _lib.ptr(kd), _lib.ptr(out4), _lib.stream_ptr()) == 0
    assert (out4.cpu().numpy() == SENTINEL).all()
    print("SITES ks%02d d%d %s " % (_ks(d), d, mode) + " ".join("%s=%.2e" % kv for kv in sorted(worst.items())))
