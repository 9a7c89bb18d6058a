"""The joint GP posterior: GP.predict_covariance, GP.sample_posterior and the C entry point scasml_gp_sample (csrc/gp_sample.hip)

    cov(x_i, y_j) = kappa(x_i, y_j) - (L^-1 K(phi, x_i))^T (L^-1 K(phi, y_j)),      out[s] = mean + Lc z(seed, sample0 + s)

against float64 NumPy written out here.  Collocation set: d = 6, 24 domain + 13 boundary points, M = 109, Mp = 128 (two 64-column blocks and a padded
tail), float16-exact so that both surrogates run.  Tolerances are not tuned to the device:
* covariance: the rule of tests/test_gpu_gp_variance.py -- two float64 host routes (solve against L; multiply by the explicit inverse of L) disagree
  by delta_host, the device must agree with the first within max(32 delta_host, 1e-13);
* sampling kernel: the componentwise bound of a length-n dot product, 8 n 2^-53 (|mean| + |Lc| |z|), against mean + tril(Lc) z with the oracle's
  normals (oracle/philox.py);
* statistics: six standard errors on every entry of the sample mean and covariance at a fixed seed (0x5CA5: the host statement alone -- oracle
  normals, NumPy product -- was checked to satisfy both bounds at that seed: largest entries 2.8 and 3.4 standard errors)."""
import ctypes as C
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

D, ND, NB = 6, 24, 13
SIZES = [(1, 1), (1, 130), (31, 65), (64, 64), (65, 31), (130, 64), (64, 1), (31, 31), (65, 130), (130, 130)]
STAT_SEED = 0x5CA5


def _idx(d):
    return [d - 1, 0, d // 2, 2, 1]


def _tolerance(delta_host):
    assert 32.0 * delta_host <= 1e-9, "the case is too ill-conditioned to expose a float32 slip: delta_host = %.3e" % delta_host
    return max(32.0 * delta_host, 1e-13)


def _points(n, seed):
    X = np.random.default_rng(seed).uniform(-0.6, 0.6, (n, D + 1)).astype(np.float16).astype(np.float32)
    X[:, -1] = np.abs(X[:, -1])
    return X


@functools.lru_cache(maxsize=None)
def _fitted(compat):
    """One fitted GP per surrogate, shared by every test below (nothing here changes it)."""
    from oracle.equation import sample_points
    from scasml_gp_amd.equations.equations import Grad_Dependent_Nonlinear
    from scasml_gp_amd.models.GP import GP_Grad_Dependent_Nonlinear
    dom, bdy = sample_points(np.random.default_rng(606), D, ND, NB)
    dom, bdy = dom.astype(np.float16).astype(np.float32), bdy.astype(np.float16).astype(np.float32)
    kw = dict(compat="reference", laplacian_idx=_idx(D)) if compat else dict(compat=None)
    gp = GP_Grad_Dependent_Nonlinear(Grad_Dependent_Nonlinear(D + 1), **kw)
    gp.GPsolver(dom, bdy, GN_steps=5)
    assert gp.phi_dim == 109 and gp._L_pad.shape[0] == 128
    return gp, dom, bdy


@functools.lru_cache(maxsize=None)
def _host(compat):
    """The device's own (older, separately tested) matrices on the host, for 130 x-points and 130 y-points: feature rows, factor, prior block; and
    the two host routes' solved rows."""
    gp, dom, bdy = _fitted(compat)
    X = np.concatenate([_points(130 - ND - NB, 1), dom, bdy]).astype(np.float32)       # the collocation points themselves among them
    Y = _points(130, 2)
    Lh = gp.cholesky_phi_phi_perturb.cpu().numpy()
    Linv = np.linalg.inv(Lh)
    out = {"X": X, "Y": Y}
    for name, P in (("X", X), ("Y", Y)):
        k = np.asarray(gp.kernel_x_t_phi(P, dom, bdy), dtype=np.float64)
        out["Va" + name], out["Vb" + name] = np.linalg.solve(Lh, k.T), Linv @ k.T
    for name, Q in (("XY", Y), ("XX", X)):
        if compat:
            out["prior" + name] = np.asarray(gp.kappa_kernel(X, Q), dtype=np.float64)
        else:
            diff2 = ((X[:, None, :].astype(np.float64) - Q[None, :, :].astype(np.float64)) ** 2).sum(-1)
            out["prior" + name] = np.exp(-gp.a * diff2 / 2.0)
    return out


# ------------------------------------------------------------------------------------------------ 1. covariance against float64 NumPy
@pytest.mark.parametrize("compat", [None, "reference"])
@pytest.mark.parametrize("n,m", SIZES)
def test_covariance_matches_float64_numpy(n, m, compat):
    gp, _, _ = _fitted(compat)
    h = _host(compat)
    got = gp.predict_covariance(h["X"][:n], h["Y"][:m])
    assert got.shape == (n, m) and got.dtype == np.float64
    cov_a = h["priorXY"][:n, :m] - h["VaX"][:, :n].T @ h["VaY"][:, :m]
    cov_b = h["priorXY"][:n, :m] - h["VbX"][:, :n].T @ h["VbY"][:, :m]
    delta_host = float(np.abs(cov_a - cov_b).max())
    err = float(np.abs(got - cov_a).max())
    print("covariance compat=%s n=%d m=%d delta_host=%.3e device-vs-A=%.3e" % (compat, n, m, delta_host, err))
    assert err <= _tolerance(delta_host)


# ------------------------------------------------------------------------------------------------ 2. structure
@pytest.mark.parametrize("compat", [None, "reference"])
def test_covariance_structure(compat):
    import torch
    gp, _, _ = _fitted(compat)
    h = _host(compat)
    X, Y = h["X"], h["Y"]
    bits = lambda a: np.ascontiguousarray(a).view(np.int64)
    full = gp.predict_covariance(X)
    assert full.shape == (130, 130)
    assert np.array_equal(bits(full), bits(full.T))                                    # exactly symmetric
    assert np.array_equal(bits(full), bits(gp.predict_covariance(X, X)))
    rect = gp.predict_covariance(X, Y)
    # a sub-selection and a permutation of the points: the same bits entry by entry
    rng = np.random.default_rng(5)
    P, Q = rng.permutation(130)[:47], rng.permutation(130)
    assert np.array_equal(bits(gp.predict_covariance(X[P])), bits(full[np.ix_(P, P)]))
    assert np.array_equal(bits(gp.predict_covariance(X[Q])), bits(full[np.ix_(Q, Q)]))
    assert np.array_equal(bits(gp.predict_covariance(X[P], Y[Q])), bits(rect[np.ix_(P, Q)]))
    # the diagonal against predict_variance: rounding only (another sum order)
    va, vb = 1.0 - (h["VaX"] ** 2).sum(0), 1.0 - (h["VbX"] ** 2).sum(0)
    delta_host = float(np.abs(va - vb).max())
    ddiag = float(np.abs(np.diag(full) - gp.predict_variance(X)[:, 0]).max())
    print("structure compat=%s diag-vs-predict_variance=%.3e delta_host=%.3e" % (compat, ddiag, delta_host))
    assert ddiag <= _tolerance(delta_host)
    # chunking is bit-invisible: row buffers of 40 rows in all (chunks of 20 points; the as-coded prior in blocks of 9 columns)
    gp.variance_buffer_bytes = 40 * 8 * gp._L_pad.shape[0]
    try:
        chunked, chunked_rect = gp.predict_covariance(X), gp.predict_covariance(X, Y[:77])
    finally:
        del gp.variance_buffer_bytes
    assert gp.variance_buffer_bytes == 1 << 30
    assert np.array_equal(bits(chunked), bits(full)) and np.array_equal(bits(chunked_rect), bits(rect[:, :77]))
    # CUDA tensor in, CUDA tensor out
    t = gp.predict_covariance(torch.from_numpy(X).cuda(), torch.from_numpy(Y).cuda())
    assert isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == torch.float64 and np.array_equal(bits(t.cpu().numpy()), bits(rect))
    assert gp.predict_covariance(X[:0]).shape == (0, 0) and gp.predict_covariance(X[:3], Y[:0]).shape == (3, 0)
    eig = np.linalg.eigvalsh(full + gp.nugget * np.eye(130))
    print("structure compat=%s eigenvalues of cov + nugget I: min %.3e max %.3e; of cov: min %.3e" % (compat, eig.min(), eig.max(), np.linalg.eigvalsh(full).min()))
    if compat is None:
        assert eig.min() > 0.0


def test_float16_rows_and_the_f16_graph_prior_mode():
    """Float16 arrays in, on an f16_graph fit: the as-coded prior follows the float16 op sequence only when x AND y are float16 arrays -- decided by
    the dtypes, so a sub-selection whose points all happen to be float16 values returns the bits of the full call."""
    from scasml_gp_amd import _lib
    from scasml_gp_amd.equations.equations import Grad_Dependent_Nonlinear
    from scasml_gp_amd.models.GP import GP_Grad_Dependent_Nonlinear
    _, dom, bdy = _fitted("reference")
    gp = GP_Grad_Dependent_Nonlinear(Grad_Dependent_Nonlinear(D + 1), compat="reference", laplacian_idx=_idx(D), f16_graph=True)
    gp.GPsolver(dom, bdy, GN_steps=5)
    bits = lambda a: np.ascontiguousarray(a).view(np.int64)
    X16, Y16 = _host("reference")["X"].astype(np.float16), _host("reference")["Y"].astype(np.float16)
    full = gp.predict_covariance(X16)
    assert full.dtype == np.float64 and np.array_equal(bits(full), bits(full.T)) and np.array_equal(bits(full), bits(gp.predict_covariance(X16, X16)))
    P = np.random.default_rng(6).permutation(130)[:51]
    assert np.array_equal(bits(gp.predict_covariance(X16[P])), bits(full[np.ix_(P, P)]))
    rect = gp.predict_covariance(X16, Y16)
    assert np.array_equal(bits(gp.predict_covariance(X16[P], Y16[P])), bits(rect[np.ix_(P, P)]))
    # float16 x against float32 y of which only the even rows are float16 values: the even rows alone give the same bits as inside the full call
    Y32 = Y16.astype(np.float32)
    Y32[1::2, :D] += np.float32(1e-4)
    mixed = gp.predict_covariance(X16, Y32)
    assert np.array_equal(bits(gp.predict_covariance(X16, Y32[0::2])), bits(mixed[:, 0::2]))
    gp.variance_buffer_bytes = 40 * 8 * gp._L_pad.shape[0]
    try:
        assert np.array_equal(bits(gp.predict_covariance(X16, Y32)), bits(mixed)) and np.array_equal(bits(gp.predict_covariance(X16)), bits(full))
    finally:
        del gp.variance_buffer_bytes
    # sample_posterior on float16 rows: predict and predict_covariance of the same float16 rows under the kernel
    import torch
    lib = _lib.load()
    draws = gp.sample_posterior(X16[:40], 7, seed=2)
    Lc = torch.eye(64, dtype=torch.float64, device="cuda")
    Lc[:40, :40] = torch.from_numpy(gp.predict_covariance(X16[:40])).cuda()
    info = torch.zeros(1, dtype=torch.int32, device="cuda")
    _lib.check(lib.scasml_cholesky(_lib.ptr(Lc), 64, float(gp.nugget), _lib.ptr(info), _lib.stream_ptr()), "cholesky")
    assert int(info.item()) == 0
    assert np.array_equal(bits(_sample(Lc, 40, gp.predict(X16[:40])[:, 0].astype(np.float64), 2, 0, 7)), bits(draws))


# ------------------------------------------------------------------------------------------------ 3. the sampling kernel alone, through the C ABI
@functools.lru_cache(maxsize=None)
def _factor_case(n):
    """(Lc on the device: the factor scasml_cholesky leaves of a random SPD matrix in an identity-padded np x np buffer, its host copy, a mean)."""
    import torch
    from scasml_gp_amd import _lib
    lib = _lib.load()
    rng = np.random.default_rng(1000 + n)
    G = rng.normal(size=(n, n))
    npad = (n + 31) // 32 * 32
    A = np.eye(npad)
    A[:n, :n] = G @ G.T / n + 0.5 * np.eye(n)
    Lc = torch.from_numpy(A).cuda()
    info = torch.zeros(1, dtype=torch.int32, device="cuda")
    _lib.check(lib.scasml_cholesky(_lib.ptr(Lc), npad, 0.0, _lib.ptr(info), _lib.stream_ptr()), "cholesky")
    assert int(info.item()) == 0
    return Lc, Lc.cpu().numpy(), rng.normal(size=n)


def _sample(Lc, n, mean, seed, sample0, S, ld=None, rows=None):
    import torch
    from scasml_gp_amd import _lib
    lib = _lib.load()
    ld, rows = ld or n, rows or S
    out = torch.full((rows, ld), 7.0, dtype=torch.float64, device="cuda")
    rc = lib.scasml_gp_sample(_lib.ptr(Lc), Lc.shape[0], n, _lib.ptr(torch.from_numpy(np.ascontiguousarray(mean)).cuda()), seed, sample0, S, _lib.ptr(out), ld,
                              _lib.stream_ptr())
    assert rc == 0, lib.scasml_last_error()
    torch.cuda.synchronize()
    return out.cpu().numpy()


def _host_normals(seed, sample0, S, n):
    from oracle import philox
    from scasml_gp_amd import _lib
    return philox.normals(seed, _lib.STREAM_GP_SAMPLE, np.arange(sample0, sample0 + S, dtype=np.uint64), 0, n).astype(np.float64)


@pytest.mark.parametrize("S", [1, 3, 64, 65])
@pytest.mark.parametrize("n", [1, 32, 33, 64, 65, 97])
def test_sampling_kernel_against_the_host_statement(n, S):
    """np = 32, 64, 96, 128: one stage, a full tile, a second point tile with one and with 33 rows; one sample, a ragged tile, a full one, two.
    A 64-bit seed and a first sample index that is no multiple of anything; a wider output buffer is not touched beyond (S, n)."""
    import torch
    seed, sample0 = 0x1234567890ABCDEF, 5
    Lc, Lh, mean = _factor_case(n)
    out = _sample(Lc, n, mean, seed, sample0, S, ld=n + 3, rows=S + 2)
    assert np.all(out[S:] == 7.0) and np.all(out[:, n:] == 7.0)
    got = out[:S, :n]
    z = _host_normals(seed, sample0, S, n)
    Lt = np.tril(Lh[:n, :n])
    want = mean[None, :] + z @ Lt.T
    bound = 8.0 * n * 2.0 ** -53 * (np.abs(mean)[None, :] + np.abs(z) @ np.abs(Lt).T)
    ratio = float((np.abs(got - want) / bound).max())
    print("sample kernel n=%d S=%d max |error| / bound = %.3e (max |error| %.3e)" % (n, S, ratio, np.abs(got - want).max()))
    assert ratio <= 1.0
    # the strict upper triangle is not read: poisoned, same bits
    poisoned = Lc.clone()
    poisoned[torch.triu(torch.ones_like(poisoned), 1).bool()] = float("nan")
    again = _sample(poisoned, n, mean, seed, sample0, S)
    assert np.array_equal(again.view(np.int64), np.ascontiguousarray(got).view(np.int64))


def test_a_draw_is_a_function_of_its_seed_and_index_alone():
    n = 97
    Lc, _, mean = _factor_case(n)
    seed = 77
    batch = _sample(Lc, n, mean, seed, 0, 65)
    for s in (0, 63, 64):
        assert np.array_equal(_sample(Lc, n, mean, seed, s, 1).view(np.int64), batch[s:s + 1].view(np.int64))
    assert np.array_equal(_sample(Lc, n, mean, seed, 10, 55).view(np.int64), np.ascontiguousarray(batch[10:]).view(np.int64))   # another split of the run
    assert np.array_equal(_sample(Lc, n, mean, seed, 0, 65).view(np.int64), batch.view(np.int64))                              # the same seed repeats
    other = _sample(Lc, n, mean, seed + 1, 0, 65)
    assert not np.any(other == batch)                                                                                           # two seeds differ
    assert not np.any(_sample(Lc, n, mean, seed + (1 << 32), 0, 65) == batch)                                                   # the seed's high word counts


def _moment_excess(x, mean, Cov):
    """Largest |sample mean - mean| and |sample covariance (about the true mean) - Cov| in units of their standard errors."""
    S = x.shape[0]
    c = x - mean[None, :]
    dev_mean = np.abs(c.mean(0)) / np.sqrt(np.diag(Cov) / S)
    dev_cov = np.abs(c.T @ c / S - Cov) / np.sqrt((np.outer(np.diag(Cov), np.diag(Cov)) + Cov ** 2) / S)
    return float(dev_mean.max()), float(dev_cov.max())


def test_sample_moments():
    n, S = 33, 4096
    Lc, Lh, mean = _factor_case(n)
    Lt = np.tril(Lh[:n, :n])
    x = _sample(Lc, n, mean, STAT_SEED, 0, S)
    em, ec = _moment_excess(x, mean, Lt @ Lt.T)
    print("sample moments n=33 S=4096 seed=0x%X: mean within %.2f, covariance within %.2f standard errors (every entry; bound 6)" % (STAT_SEED, em, ec))
    assert em <= 6.0 and ec <= 6.0


# ------------------------------------------------------------------------------------------------ 4. sample_posterior end to end
@pytest.mark.parametrize("compat", [None, "reference"])
def test_sample_posterior_end_to_end(compat):
    import torch
    from scasml_gp_amd import _lib
    lib = _lib.load()
    gp, dom, bdy = _fitted(compat)
    X = _host(compat)["X"][:70]                                                        # np = 96
    draws = gp.sample_posterior(X, 130, seed=9, sample0=3)
    assert isinstance(draws, np.ndarray) and draws.shape == (130, 70) and draws.dtype == np.float64 and np.all(np.isfinite(draws))
    # = mean + the kernel's output on the class's own covariance
    mean = gp.predict(X)[:, 0].astype(np.float64)
    Lc = torch.eye(96, dtype=torch.float64, device="cuda")
    Lc[:70, :70] = torch.from_numpy(gp.predict_covariance(X)).cuda()
    info = torch.zeros(1, dtype=torch.int32, device="cuda")
    _lib.check(lib.scasml_cholesky(_lib.ptr(Lc), 96, float(gp.nugget), _lib.ptr(info), _lib.stream_ptr()), "cholesky")
    assert int(info.item()) == 0
    assert np.array_equal(_sample(Lc, 70, mean, 9, 3, 130).view(np.int64), draws.view(np.int64))
    # sample0 continues a stream; the chunks n_samples is walked in are invisible (below: 128 draws per launch)
    assert np.array_equal(gp.sample_posterior(X, 100, seed=9, sample0=33), draws[30:])
    gp.variance_buffer_bytes = 8 * 96 * 96
    try:
        assert np.array_equal(gp.sample_posterior(X, 130, seed=9, sample0=3), draws)
        with pytest.raises(ValueError, match="n <= 96"):                               # the n x n factor must fit the buffer
            gp.sample_posterior(_host(compat)["X"][:97], 2)
    finally:
        del gp.variance_buffer_bytes
    t = gp.sample_posterior(torch.from_numpy(X).cuda(), 5, seed=9, sample0=3)
    assert isinstance(t, torch.Tensor) and t.is_cuda and np.array_equal(t.cpu().numpy(), draws[:5])
    assert gp.sample_posterior(X, 0).shape == (0, 70)
    with pytest.raises(ValueError):
        gp.sample_posterior(X, -1)
    # jitter.  At this size no small non-negative jitter fails, for either surrogate: measured on the device, the smallest eigenvalue of the
    # 130-point covariance is 1.5e-3 (documented) / 2.3e-3 (as coded), and these 70 points are a principal submatrix of it -- so jitter = 0 is
    # asserted to succeed.  The refusal is exercised with a jitter that is too small by construction: cov[0, 0] <= kappa(x, x) = 1, so the
    # first pivot of cov - 1.5 I is negative.
    assert np.all(np.isfinite(gp.sample_posterior(X, 3, seed=9, jitter=0.0)))
    with pytest.raises(ValueError, match="jitter = -1.5"):
        gp.sample_posterior(X, 3, seed=9, jitter=-1.5)


def test_sample_posterior_rebuilds_the_factor_once_after_load_state_dict():
    from scasml_gp_amd.equations.equations import Grad_Dependent_Nonlinear
    from scasml_gp_amd.models.GP import GP_Grad_Dependent_Nonlinear
    gp, _, _ = _fitted("reference")
    X = _host("reference")["X"][:40]
    fresh = GP_Grad_Dependent_Nonlinear(Grad_Dependent_Nonlinear(D + 1), compat="reference", laplacian_idx=_idx(D))
    fresh.load_state_dict(gp.state_dict())
    assert getattr(fresh, "_L_pad", None) is None
    calls = []
    inner = fresh.kernel_phi_phi
    fresh.kernel_phi_phi = lambda *a: (calls.append(1), inner(*a))[1]
    first = fresh.sample_posterior(X, 6, seed=4)
    assert len(calls) == 1 and np.array_equal(first, gp.sample_posterior(X, 6, seed=4))
    fresh.sample_posterior(X, 6, seed=5)
    fresh.predict_covariance(X)
    assert len(calls) == 1
