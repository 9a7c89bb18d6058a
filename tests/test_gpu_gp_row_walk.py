"""The two walks GP's feature-row paths share, and the one intake of a caller's points (scasml_gp_amd/models/GP.py):

* GP._cross_rows walks every set of rows at most ``cross_rows_per_call`` rows per scasml_gp_cross_rows call.  The library's limit, 65535 * 16 rows,
  takes more than a million points to reach, so the cap is lowered on the instance here: 100 rows under a cap of 48 are three calls with a ragged
  last one, and must give the bits of the one call the default cap makes -- for the cross-kernel builders (op 4 has M (d+1) doubles per row, so an
  offset slip shows), predict_variance and predict_covariance;
* predict_variance / predict_covariance walk their points in chunks under ``variance_buffer_bytes`` on top of it: both walks together, both ragged;
* GP._rows_device: the (n, d+1) shape error, float16 against float32 arrays of the same values, NumPy in / NumPy out and tensor in / tensor out.

Collocation set of tests/test_gpu_gp_posterior.py: d = 6, 24 domain + 13 boundary float16-exact points, M = 109, Mp = 128.  Every comparison is bit
for bit: each row is a function of its own point alone, so no tolerance enters."""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

D, ND, NB = 6, 24, 13
N_INF_ARG = 11                      # scasml_gp_cross_rows(d, a, x_dom, n_dom, x_bdy, n_bdy, idx, round16, surrogate, op, x_inf, n_inf, ...)


def _points(n, seed):
    X = np.random.default_rng(seed).uniform(-0.6, 0.6, (n, D + 1)).astype(np.float16).astype(np.float32)
    X[:, -1] = np.abs(X[:, -1])
    return X


@functools.lru_cache(maxsize=None)
def _fitted(compat):
    """One fitted GP per surrogate, shared by every test below (they change instance attributes only, and take them off again)."""
    from oracle.equation import sample_points
    from scasml_gp_amd.equations.equations import Grad_Dependent_Nonlinear
    from scasml_gp_amd.models.GP import GP_Grad_Dependent_Nonlinear
    dom, bdy = sample_points(np.random.default_rng(606), D, ND, NB)
    dom, bdy = dom.astype(np.float16).astype(np.float32), bdy.astype(np.float16).astype(np.float32)
    kw = dict(compat="reference", laplacian_idx=[D - 1, 0, D // 2, 2, 1]) if compat else dict(compat=None)
    gp = GP_Grad_Dependent_Nonlinear(Grad_Dependent_Nonlinear(D + 1), **kw)
    gp.GPsolver(dom, bdy, GN_steps=5)
    assert gp.phi_dim == 109 and gp._L_pad.shape[0] == 128
    return gp, dom, bdy


def _bits(a):
    """The array's bytes as integers of its own width (int64 for the float64 results, int16 for the as-coded builders' float16 rows)."""
    a = np.ascontiguousarray(a)
    return a.view("i%d" % a.dtype.itemsize)


class _CrossRowCounter:
    """The library, with the row count of every scasml_gp_cross_rows call noted."""

    def __init__(self, lib):
        self._lib, self.rows = lib, []

    def __getattr__(self, name):
        fn = getattr(self._lib, name)
        if name != "scasml_gp_cross_rows":
            return fn

        def counted(*args):
            self.rows.append(int(args[N_INF_ARG]))
            return fn(*args)
        return counted


@pytest.fixture
def cross_row_calls(monkeypatch):
    from scasml_gp_amd import _lib
    counter = _CrossRowCounter(_lib.load())
    monkeypatch.setattr(_lib, "load", lambda: counter)
    return counter.rows


def _results(gp, dom, bdy, X, Y):
    return {"kernel_x_t_phi": gp.kernel_x_t_phi(X, dom, bdy), "laplacian_x_t_kernel_x_t_phi": gp.laplacian_x_t_kernel_x_t_phi(X, dom, bdy),
            "dx_t_kernel_x_t_phi": gp.dx_t_kernel_x_t_phi(X, dom, bdy), "predict_variance": gp.predict_variance(X),
            "predict_covariance(x)": gp.predict_covariance(X), "predict_covariance(x, y)": gp.predict_covariance(X, Y)}


@pytest.mark.parametrize("compat", [None, "reference"])
def test_a_shrunken_row_cap_returns_the_same_bits(compat, cross_row_calls):
    from scasml_gp_amd.models.GP import GP
    gp, dom, bdy = _fitted(compat)
    X, Y = _points(100, 1), _points(70, 2)
    want = _results(gp, dom, bdy, X, Y)
    assert want["dx_t_kernel_x_t_phi"].shape == (100, 109, D + 1) and want["predict_covariance(x, y)"].shape == (100, 70)
    assert set(cross_row_calls) <= {100, 70}                                          # the default cap: every set of rows in one call
    gp.cross_rows_per_call = 48
    try:
        del cross_row_calls[:]
        gp.kernel_x_t_phi(X, dom, bdy)
        assert cross_row_calls == [48, 48, 4]                                          # three calls, a ragged last one
        got = _results(gp, dom, bdy, X, Y)
        assert set(cross_row_calls) == {48, 4, 22}                                     # 70 = 48 + 22
    finally:
        del gp.cross_rows_per_call
    assert gp.cross_rows_per_call == GP.cross_rows_per_call == 65535 * 16
    for name in want:
        assert got[name].dtype == want[name].dtype and np.array_equal(_bits(got[name]), _bits(want[name])), name


@pytest.mark.parametrize("compat", [None, "reference"])
def test_the_row_cap_and_the_buffer_chunks_together(compat, cross_row_calls):
    """variance_buffer_bytes of 40 rows: predict_variance walks 100 = 40 + 40 + 20 points, and a cap of 16 splits every one of those chunks again
    (40 = 16 + 16 + 8, 20 = 16 + 4); predict_covariance's two buffers take 20 rows each (20 = 16 + 4)."""
    gp, _, _ = _fitted(compat)
    X = _points(100, 1)
    var, cov = gp.predict_variance(X), gp.predict_covariance(X)
    gp.cross_rows_per_call = 16
    gp.variance_buffer_bytes = 40 * 8 * gp._L_pad.shape[0]
    try:
        del cross_row_calls[:]
        var_chunked = gp.predict_variance(X)
        assert cross_row_calls == [16, 16, 8, 16, 16, 8, 16, 4]
        cov_chunked = gp.predict_covariance(X)
    finally:
        del gp.cross_rows_per_call, gp.variance_buffer_bytes
    assert gp.cross_rows_per_call == 65535 * 16 and gp.variance_buffer_bytes == 1 << 30
    assert np.array_equal(_bits(var_chunked), _bits(var)) and np.array_equal(_bits(cov_chunked), _bits(cov))


@pytest.mark.parametrize("compat", [None, "reference"])
def test_the_intake_of_points(compat):
    import torch
    gp, dom, bdy = _fitted(compat)
    wrong = np.zeros((5, D), dtype=np.float32)
    for call in (gp.predict_variance, gp.predict_covariance, lambda x: gp.predict_covariance(_points(3, 3), x)):
        with pytest.raises(ValueError, match=r"points must have shape \(n, 7\)"):
            call(wrong)
        with pytest.raises(ValueError, match=r"points must have shape \(n, 7\)"):
            call(torch.from_numpy(wrong).cuda())
    # the cross-kernel builders take any array of n (d+1) entries as n rows (kappa and its kin hand them single vectors); 30 entries are no rows
    X = _points(9, 4)
    rows = gp.kernel_x_t_phi(X, dom, bdy)
    assert np.array_equal(_bits(gp.kernel_x_t_phi(X.reshape(-1), dom, bdy)), _bits(rows))
    with pytest.raises((ValueError, RuntimeError)):
        gp.kernel_x_t_phi(wrong, dom, bdy)
    # NumPy in, NumPy out; CUDA tensor in, CUDA tensor out; the same bits
    Xt = torch.from_numpy(X).cuda()
    for host, dev in ((rows, gp.kernel_x_t_phi(Xt, dom, bdy)), (gp.predict_variance(X), gp.predict_variance(Xt)),
                      (gp.predict_covariance(X), gp.predict_covariance(Xt)), (gp.predict_covariance(X, X[:4]), gp.predict_covariance(Xt, Xt[:4]))):
        assert isinstance(host, np.ndarray) and isinstance(dev, torch.Tensor) and dev.is_cuda
        assert np.array_equal(_bits(dev.cpu().numpy()), _bits(host))


def test_float16_arrays_of_the_documented_surrogate():
    """The documented operators round nothing, so the dtype the points arrive in cannot matter: float16 arrays give the bits of their float32 values."""
    gp, _, _ = _fitted(None)
    X = _points(33, 5)
    assert np.array_equal(_bits(gp.predict_variance(X.astype(np.float16))), _bits(gp.predict_variance(X)))
