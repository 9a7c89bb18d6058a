"""PDE-constrained Gaussian-process surrogate with the reference's call surface
(models/GP.py: ``GP`` :8-692, ``GP_Grad_Dependent_Nonlinear`` :693-769), on libscasml_hip.

What runs where:
* Gram K(phi,phi) in closed form (25 blocks, float64) ............ scasml_gp_gram      (:182-258)
* Cholesky of K + nugget*I (replaces the SVD factor, :260-267) ... scasml_cholesky
* K_p^{-1} by two blocked triangular solves, Newton step solves .. scasml_trsm_lower  (:439,533,599)
* the Newton objective as a method of its own (:430-444) ....... GP.loss_function -> scasml_gp_newton_b, scasml_trsm_lower
* the Newton iteration (:487-604): with A = K_p^{-1} explicit, gradient and Hessian of b(sol)^T A b(sol)
  are block-wise elementwise expressions (b is affine except for the product z1*z5 in F, :705-719), so
  no autodiff and no per-iteration GEMM is needed ........... scasml_gp_newton_b / _gemv / _gp_newton_system
* predict / compute_gradient / compute_PDE_loss (:653-687, 746-769) .. scasml_gp_eval, scasml_gp_gradient
* log marginal likelihood, its gradient in (log sigma, log nugget) and a fit of the two (no counterpart: :25-26 hard-code them; compat=None only)
  .............................................................. scasml_chol_logdet, scasml_gp_gram_da_contract
* posterior draws as functions (no counterpart; compat=None only): GP.sample_functions -> GPFunctionDraws ... scasml_gp_rff_functionals,
  scasml_gp_rff_noise, scasml_trsm_lower, scasml_gp_cross_rows, scasml_gemm_nt_sub; their gradients (GPFunctionDraws.gradient) and the float64
  gradient of the mean (GP.posterior_mean_gradient) ... scasml_gp_rff_gradient, scasml_gp_cross_rows (op 0, op 2), scasml_gemm_nt_sub
* posterior covariance of [u, Lap u, dt u, div u] at a point and the delta-method variance of the PDE residual (no counterpart; compat=None only):
  GP.predict_functional_covariance, GP.predict_residual_variance ... scasml_gp_cross_rows (op 0 .. 3), scasml_gp_functional_covariance, scasml_gemm_nt_sub

Two surrogates (``compat``):
* ``None``: the operators the reference documents -- exact Laplacian features, no float16 rounding.
* ``"reference"`` (default): the surrogate the reference's code actually builds: the 5-index
  Hutchinson "Laplacian" on a cyclically shifted argument (:28-39, 87-105, 119-179) with a caller-supplied index set
  (``laplacian_idx``; the reference's comes from JAX threefry), every kernel entry rounded to float16 (:43), K_p rounded
  to float16 for the right_vector solve (:267-268, 599), z4 rounded to float16 (:719), u_hat and eps_PDE returned as float16
  values (:671, 769).  Evaluation runs on the matrix cores (csrc/gp_eval_compat_mfma.hip: the three shifted geometries are one
  x.y product against three cyclic shifts of the collocation rows) when the collocation points are exactly float16 -- the
  reference's are -- and in float64 (csrc/gp_compat.hip, ``compat_eval = "float64"``) otherwise; Gram, gradient and the CPU
  statement (oracle/gp_compat.py) are float64.  ``laplacian_idx`` may be the five indices or the name of the Threefry counter
  layout ("original" / "partitionable") with which the reference's own draw is recomputed (scasml_gp_amd/threefry.py).
* ``"reference-geometry"`` (opt-in): the SAME fit (Gram, K_p, right_vector of ``"reference"``) evaluated on the hot path without the float16
  rounding of every kernel entry, which lets the four sums factor per pair geometry (13 + 9 + 5 vector instructions per pair instead of
  27 + 13 + 13), and with the evaluation point's coordinates entering the x.y products as ONE float16 plane (half the MFMAs).  On the
  reference's own experiments (d = 20 .. 80) GP relative L2 moves by <= 1e-5 and ScaSML by <= 3e-5 against ``"reference"``
  (profiles/r04_eval_rounding_study.txt); u_hat and eps_PDE still leave as float16 values (:671, 769).
Remaining deviations in both: Newton start at 0 instead of 1e-3*N(0,1) from PRNGKey(0) (:501); Cholesky instead of
the SVD factor, so the float16 rounding of L itself (:266) has no counterpart (no measurable effect).
Which triangle: every factorisation here (scasml_cholesky, dist_gp.DistCholesky, the oracle's eigh) reads the LOWER triangle of K, i.e. it
factors tril(K) + tril(K, -1)^T.  With one rounding per entry K is symmetric and nothing is dropped.  Under ``f16_graph`` it is not (the
(dt, div) entry and its mirror are two different float16 rounding sequences, up to 1.4e-3 relative apart): the reference's SVD (:260) and
jnp.linalg.solve (:599) consume both halves, this build the lower one; kernel_phi_phi still returns the matrix as coded, asymmetric.  The GP
error on the reference's logs is unaffected to the digits they print (tests/test_gpu_f16_graph.py pins the triangle and the logged numbers).
"""
import ctypes as C
import os

import numpy as np

from .. import _lib


def _round_up(v, m):
    return (v + m - 1) // m * m


def _f16_exact(*xs):
    """Whether every entry of every array (torch tensors, NumPy arrays) is a float16 value, in the array's own dtype."""
    import torch
    ts = (x if isinstance(x, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(x)) for x in xs)
    return all(bool((t.half().to(t.dtype) == t).all()) for t in ts)


def _maximize_bounded(fun, x0, lo, hi, gtol, max_iter):
    """Maximise ``fun`` over the box lo <= x <= hi in a handful of variables (GP.optimize_hyperparameters: one or two log-parameters).
    fun(x) -> (value, gradient), or None where the function is undefined (taken as a rejected trial point).

    Projected BFGS on -fun: variables that sit on a bound with the gradient pushing outward are held, the others move along -H g (the first step
    and every restart: steepest ascent), no step longer than 1 in any variable (a factor e in a log-parameter), trial points clipped into the
    box, Armijo backtracking with a safeguarded quadratic fit, the inverse-Hessian update skipped when the curvature along the step is not
    positive.  Stops when max |g| over the variables not held is <= gtol (converged), after max_iter iterations or when the line search finds
    no increase.  Returns (x, value, gradient, evaluations, iterations, converged)."""
    lo, hi = np.asarray(lo, dtype=np.float64), np.asarray(hi, dtype=np.float64)
    x = np.clip(np.asarray(x0, dtype=np.float64), lo, hi)
    res = fun(x)
    if res is None:
        raise ValueError("the function is undefined at the start")
    f, g = -float(res[0]), -np.asarray(res[1], dtype=np.float64)
    evals, iters, H = 1, 0, None
    while True:
        free = ~(((x <= lo) & (g > 0.0)) | ((x >= hi) & (g < 0.0)))
        if not free.any() or float(np.abs(g[free]).max()) <= gtol:
            return x, -f, -g, evals, iters, True
        if iters >= max_iter:
            return x, -f, -g, evals, iters, False
        iters += 1
        p = -(H @ g) if H is not None else -g
        p[~free] = 0.0
        if H is None or float(p @ g) >= 0.0:                 # no model yet, or not a descent direction: restart along the projected gradient
            H = None
            p = np.where(free, -g, 0.0)
        big = float(np.abs(p).max())
        if big > 1.0:
            p = p / big
        t, accepted = 1.0, None
        for _ in range(30):
            xn = np.clip(x + t * p, lo, hi)
            step = xn - x
            if not step.any():
                break
            res = fun(xn)
            evals += 1
            slope = float(g @ step)
            if res is not None and -float(res[0]) <= f + 1e-4 * slope:
                accepted = (xn, -float(res[0]), -np.asarray(res[1], dtype=np.float64))
                break
            # minimiser of the parabola through f, slope and the rejected value, kept inside [0.1 t, 0.5 t]
            tq = 0.5 * t if res is None else -slope * t / (2.0 * (-float(res[0]) - f - slope))
            t = min(max(tq, 0.1 * t), 0.5 * t) if np.isfinite(tq) and tq > 0.0 else 0.5 * t
        if accepted is None:
            return x, -f, -g, evals, iters, False
        xn, fn, gn = accepted
        s, y = xn - x, gn - g
        sy = float(s @ y)
        if sy > 1e-12 * float(np.linalg.norm(s) * np.linalg.norm(y)):
            if H is None:
                H = np.eye(len(x)) * (sy / float(y @ y))
            rho = 1.0 / sy
            V = np.eye(len(x)) - rho * np.outer(s, y)
            H = V @ H @ V.T + rho * np.outer(s, s)
        x, f, g = xn, fn, gn


class GPFunctionDraws(object):
    """Posterior draws of a GP as FUNCTIONS (GP.sample_functions; pathwise conditioning, Wilson et al. 2020): draw s is
        post_s(x) = f_s(x) + k(x, phi)^T right_vectors[s],     (L post_s)(x) = (L f_s)(x) + (L_x k)(x, phi)^T right_vectors[s],   L in {I, Lap, dt, div}
    with f_s the random-Fourier-feature prior draw of scasml_gp_rff_functionals.  The object holds the (S, M) right vectors and the five scalars that
    name the prior draws (d, a, n_features, seed, sample0) -- not the features, which the kernel regenerates from Philox at every evaluation -- and the
    GP whose collocation points the cross rows are taken against.  Draw s is a function of (model, seed, sample0 + s, n_features) alone: the points may
    be split, permuted or revisited freely and every value comes back bit for bit."""

    def __init__(self, gp, right_vectors, n_features, seed, sample0):
        torch = _lib.require_gpu()
        self.gp, self.right_vectors = gp, right_vectors
        self.d, self.a, self.n_features, self.seed, self.sample0 = gp.d, gp.a, int(n_features), int(seed), int(sample0)
        S, M = right_vectors.shape
        # -right_vectors in rows of Mp columns, the padding zero: what scasml_gemm_nt_sub takes (C -= rows B^T adds the data term)
        self._neg = torch.zeros((S, _round_up(max(M, 1), 32)), dtype=torch.float64, device="cuda")
        self._neg[:, :M] = -right_vectors

    @property
    def n_samples(self):
        return self.right_vectors.shape[0]

    def _evaluate(self, x, ops):
        """(S, n, len(ops)) float64 on the device, and whether x was a NumPy array."""
        torch = _lib.require_gpu()
        lib = _lib.load()
        gp = self.gp
        xi, was_numpy, _ = gp._rows_device(x)
        S, n, Mp = self.n_samples, xi.shape[0], self._neg.shape[1]
        out = torch.empty((S, n, len(ops)), dtype=torch.float64, device="cuda")
        if S == 0 or n == 0:
            return out, was_numpy
        s = _lib.stream_ptr()
        chunk = int(max(1, min(gp.variance_buffer_bytes // (8 * Mp), gp.cross_rows_per_call, n)))
        rows = torch.zeros((chunk, Mp), dtype=torch.float64, device="cuda")      # columns M .. Mp stay zero: the cross rows fill 0 .. M
        for lo in range(0, n, chunk):
            xc = xi[lo:lo + chunk]
            c = xc.shape[0]
            prior = gp._rff_functionals(xc, self.n_features, self.seed, self.sample0, S)       # (S, c, 4)
            vals = prior[:, :, list(ops)].permute(1, 2, 0).contiguous()                        # (c, ops, S): one (c x S) block per operator
            for k, op in enumerate(ops):
                gp._cross_rows(gp._xd, gp._xb, op, xc, rows, Mp, 0)
                block = vals[:, k, :]
                _lib.check(lib.scasml_gemm_nt_sub(_lib.ptr(block), vals.stride(0), c, S, _lib.ptr(rows), Mp, _lib.ptr(self._neg), Mp, Mp, 0, 0, 0, s),
                           "gemm_nt_sub")
            out[:, lo:lo + c, :] = vals.permute(2, 0, 1)
        return out, was_numpy

    def predict(self, x):
        """(S, n) float64: every draw at the points x (NumPy in, NumPy out; CUDA tensor in, CUDA tensor out).  The mean part is the float64 statement
        k(x)^T right_vector, not the bf16 evaluation of GP.predict."""
        out, was_numpy = self._evaluate(x, (0,))
        out = out[:, :, 0].contiguous()
        return out.cpu().numpy() if was_numpy else out

    def functionals(self, x):
        """(S, n, 4) float64: u, Lap u, dt u and div u (= sum_k d_k u, as everywhere in this library) of every draw at the points x."""
        out, was_numpy = self._evaluate(x, (0, 1, 2, 3))
        return out.cpu().numpy() if was_numpy else out

    def gradient(self, x):
        """(S, n, d+1) float64: the gradient of every draw at the points x, time derivative last (NumPy in, NumPy out; CUDA tensor in, CUDA tensor
        out): the prior term by scasml_gp_rff_gradient, the data term by GP._data_gradient (the gradient of k(x, phi)^T right_vectors[s] without the
        n x M x (d+1) rows of scasml_gp_cross_rows' op 4).  Component d is functionals(x)[..., 2] and the first d sum to functionals(x)[..., 3], to
        rounding."""
        gp = self.gp
        if gp.compat == "reference":
            raise ValueError("pathwise draws need compat=None: the as-coded matrix is not the Gram of one kernel and has no spectral density")
        xi, was_numpy, _ = gp._rows_device(x)
        out = gp._data_gradient(xi, self._neg, lambda xc: gp._rff_gradient(xc, self.n_features, self.seed, self.sample0, self.n_samples))
        return out.cpu().numpy() if was_numpy else out


class GP(object):
    '''Gaussian Kernel Solver for high dimensional PDE'''

    def __init__(self, equation, compat="reference", laplacian_idx="partitionable", f16_graph=False):
        """compat="reference" (default): the surrogate the reference's code builds, with its own Hutchinson index draw
        (laplacian_idx: five indices, or the Threefry counter layout the draw is recomputed with -- "partitionable" reproduces the
        reference's logged errors, "original" is jax < 0.5).  compat=None: the operators the reference documents."""
        if compat == "exact":
            compat = None
        # "reference-geometry": the fit of "reference", the hot evaluation without the per-entry float16 roundings (module docstring)
        self.eval_geometry = compat == "reference-geometry"
        if self.eval_geometry:
            compat = "reference"
        if compat not in (None, "reference"):
            raise ValueError("compat must be 'reference', 'reference-geometry' or None")
        if compat == "reference" and equation.n_input - 1 < 5:
            raise ValueError("compat='reference' draws five distinct Hutchinson indices from d = %d < 5 coordinates (the reference's "
                             "random.choice(..., replace=False) fails there too); use compat=None" % (equation.n_input - 1))
        self.compat = compat
        # f16_graph (opt-in, compat="reference"): on FLOAT16 rows -- the collocation points in the fit, float16 arrays handed to predict /
        # compute_PDE_loss -- the nine Laplacian-free kernel entries follow the reference's float16 op sequence (kappa in float16 arithmetic, its
        # derivative kernels reverse-mode autodiff through it; csrc/gp_compat.hip f16_graph_blocks, oracle: OracleGPCompat(f16_graph=2)) instead of
        # one rounding per entry.  Brings the GP's relative L2 on the reference's experiments from <= 1e-4 to ~1e-5 of the logged numbers.  The
        # solvers' hot evaluation (float32 tree points) is unaffected.
        self.f16_graph = bool(f16_graph) and compat == "reference"
        self._f16_extra = _lib.ROUND16_F16_LAP if os.environ.get("SCASML_GP_F16_LEVEL") == "3" else 0     # exploratory
        self.laplacian_idx = None
        if compat == "reference":
            if isinstance(laplacian_idx, str):                   # the reference's own draw, models/GP.py:35
                from ..threefry import reference_laplacian_idx
                laplacian_idx = reference_laplacian_idx(equation.n_input - 1, laplacian_idx)
            idx = np.asarray(laplacian_idx if laplacian_idx is not None else [], dtype=np.int32).reshape(-1)
            if idx.size != 5 or len(set(idx.tolist())) != 5 or idx.min() < 0 or idx.max() >= equation.n_input - 1:
                raise ValueError("compat='reference' needs laplacian_idx: five distinct indices in [0, d) "
                                 "(models/GP.py:35 draws them from PRNGKey(0))")
            self.laplacian_idx = np.ascontiguousarray(idx)
        self.equation = equation
        equation.geometry()
        self.T = equation.T
        self.t0 = equation.t0
        self.n_input = equation.n_input
        self.n_output = equation.n_output
        self.d = self.n_input - 1
        self.sigma = equation.sigma() * np.sqrt(self.d)      # models/GP.py:25
        self.nugget = 1e-2                                   # :26
        self.right_vector = None
        # arithmetic of x.y in the fused evaluation: 3 = three bf16 planes on the bf16 matrix cores
        # (products exact to fp32), 22 = two fp16 planes (22-bit products, half the MFMAs), 2 = two bf16
        # planes (~2^-16 per product), 0 = fp32-input MFMA
        self.eval_split = int(os.environ.get("SCASML_GP_SPLIT", "22"))
        # compat="reference" evaluation kernel: "mfma" (matrix cores; needs float16-exact collocation points, else float64 is
        # used) or "float64" (one wavefront per point, rounding decided exactly as the NumPy statement decides it)
        self.compat_eval = os.environ.get("SCASML_GP_COMPAT_EVAL", "mfma")
        # round16 argument of the compat evaluation (_lib.ROUND16_*): entries rounded (:43, 55-179) and outputs rounded (:671, 769) are the
        # reference's code (3); compat="reference-geometry" drops the entry rounding for one float16 plane of the evaluation point (6)
        self.eval_round16 = int(os.environ.get("SCASML_GP_EVAL_ROUND16", _lib.ROUND16_OUTPUTS | (
            _lib.ROUND16_ONE_PLANE if self.eval_geometry else _lib.ROUND16_ENTRIES)))
        self.profile = False            # bench.py: HIP-event time of every training stage into self.stage_ms
        self.stage_ms = {}

    def _stage(self, name, fn):
        """Run one training stage; with self.profile bracket it with HIP events on the launch stream."""
        if not self.profile:
            return fn()
        torch = _lib.require_gpu()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        out = fn()
        e1.record()
        e1.synchronize()
        self.stage_ms[name] = self.stage_ms.get(name, 0.0) + e0.elapsed_time(e1)
        return out

    # ------------------------------------------------------------------ device helpers
    def _check_rows(self, x):
        if x.dim() != 2 or x.shape[1] != self.d + 1:
            raise ValueError("points must have shape (n, %d), got %s" % (self.d + 1, tuple(x.shape)))

    def _rows_device(self, x, flat=False):
        """(n, d+1) numpy / torch -> (float32 contiguous CUDA rows, was_numpy, float16 rows): the one intake of a caller's points.  ``float16
        rows`` says the caller's array was float16 -- numpy or torch alike -- i.e. rows on which the reference's kernels are float16 arithmetic
        (f16_graph).  flat (the cross-kernel builders): any array of n (d+1) entries is taken as n rows."""
        torch = _lib.require_gpu()
        was_numpy = not isinstance(x, torch.Tensor)
        f16_rows = (np.asarray(x).dtype == np.float16) if was_numpy else x.dtype == torch.float16
        xi = torch.from_numpy(np.ascontiguousarray(np.asarray(x), dtype=np.float32)) if was_numpy else x
        xi = xi.to(device="cuda", dtype=torch.float32).contiguous()
        if flat:
            xi = xi.reshape(-1, self.d + 1)
        self._check_rows(xi)
        return xi, was_numpy, bool(f16_rows)

    def _points_device(self, x):
        """(n, d+1) numpy / torch -> ((n, kp) float32 CUDA rows (X, t, zero pad), was_numpy, host bound, float16 rows).  The largest
        |coordinate| of a host array is taken on the host, from its float32 values, so that the evaluation need not read it back from the
        device (None for device tensors).  Both travel as return values: nothing about one call is parked on the instance."""
        torch = _lib.require_gpu()
        xt, was_numpy, f16_rows = self._rows_device(x)
        bound = None
        if was_numpy:
            arr = np.asarray(x, dtype=np.float32)
            bound = float(np.abs(arr).max()) if arr.size else 0.0
        kp = int(_lib.load().scasml_point_stride(self.d))
        pts = torch.zeros((xt.shape[0], kp), dtype=torch.float32, device="cuda")
        pts[:, :self.d + 1] = xt
        return pts, was_numpy, bound, f16_rows

    @property
    def a(self):
        """The kernel's scale a = 1 / sigma^2 (models/GP.py:25, 41-43)."""
        return self._a_of(self.sigma)

    @staticmethod
    def _a_of(sigma):
        return 1.0 / float(sigma) ** 2

    def _fp16_in_range(self, x_bound):
        """The fp16 planes' range rule: 0.72 a |x|^2 with |x_k| <= x_bound (0 = the default 2) stays below 3e4 (scasml_gp_model.x_bound)."""
        xb = x_bound if x_bound > 0 else 2.0
        return 0.7213 * self.a * xb * xb * (self.d + 1) <= 3.0e4

    def _f16_graph_rows(self, f16_rows):
        """f16_graph applies: float16 rows against float16 collocation points of the as-coded fit."""
        return self.f16_graph and f16_rows and getattr(self, "_colloc_is_f16", False)

    def _fp16_planes(self, f16_rows=False):
        """Whether the kernel _eval_rows chooses may carry the rows in fp16 planes, i.e. needs their coordinate bound."""
        if self.compat is None:
            return int(self.eval_split) == 22
        return self.compat_eval == "mfma" and not self._f16_graph_rows(f16_rows)

    def _gram_bits(self, x_dom, x_bdy, f16_rows=True):
        """round16 of the as-coded Gram, Gram rows and cross rows: entries rounded; f16_graph on float16 rows and collocation points: float16 ops.
        The documented operators round nothing: 0."""
        if self.compat is None:
            return 0
        graph = self.f16_graph and f16_rows and _f16_exact(x_dom, x_bdy)
        return _lib.ROUND16_ENTRIES | (_lib.ROUND16_F16_OPS | self._f16_extra if graph else 0)

    def _require_trained(self):
        if self.right_vector is None:
            raise _lib.ScasmlError("GP is not trained: call GPsolver(x_domain, x_boundary) first")

    @property
    def _idx_ptr(self):
        """The Hutchinson index set as the library takes it: its pointer for the as-coded surrogate, None for the documented operators."""
        return self.laplacian_idx.ctypes.data_as(C.c_void_p) if self.compat == "reference" else None

    def _f64_model(self):
        """The fit as the as-coded float64 kernels take it: collocation columns, n_dom, n_bdy, ldc, right_vector, Hutchinson indices."""
        self._require_trained()
        return (_lib.ptr(self._colloc_t), self.N_domain, self.N_boundary, self.N_domain + self.N_boundary, _lib.ptr(self._rv_dev), self._idx_ptr)

    def _device_model(self, x_bound=0.0):
        self._require_trained()
        m = _lib.GpModel()
        m.x_bound = float(x_bound)
        m.d, m.n_dom, m.n_bdy, m.n_pad = self.d, self.N_domain, self.N_boundary, self._n_pad
        m.kp = self._colloc.shape[1]
        # a stated bound out of range demotes the fp16 x 2 split to bf16 x 3; without one (0) the library refuses what 2 would break
        m.split = 3 if int(self.eval_split) == 22 and x_bound > 0 and not self._fp16_in_range(x_bound) else int(self.eval_split)
        m.a = self.a
        m.sigma_eq = float(self.equation.sigma())
        m.mu_eq = float(self.equation.mu())
        m.eq_id = int(self.equation.eq_id)
        m.colloc, m.colloc_frag, m.coef = self._colloc.data_ptr(), self._frag.data_ptr(), self._coef.data_ptr()
        m.colloc_bf16 = self._bf16.data_ptr()
        m.colloc_is_f16 = int(self._colloc_is_f16)
        return m

    def _eval_device(self, pts, host_bound=None, f16_rows=False):
        """Caller-supplied points: their coordinate bound (``host_bound`` of _points_device for host arrays; one reduction + read for device
        tensors) lets far-out rows fall back to the bf16 x 3 arithmetic instead of overflowing the fp16 planes."""
        torch = _lib.require_gpu()
        out = torch.empty((pts.shape[0], 4), dtype=torch.float32, device="cuda")
        xb = (host_bound if host_bound is not None else float(pts.abs().max())) if pts.shape[0] and self._fp16_planes(f16_rows) else 0.0
        self._eval_rows(pts, pts.shape[0], 0, None, out, x_bound=max(xb, 2.0) if xb > 0 else 0.0, f16_rows=f16_rows)
        return out

    def _eval_rows(self, pts, n_rows, rows_per_site, kinds, out4, x_bound=0.0, order=None, f16_rows=False):
        """(u_hat, div u_hat, eps_PDE, dt u_hat) of the first n_rows point rows into out4: the one place the solvers and
        predict / compute_PDE_loss reach the evaluation kernels, and where the kernel is chosen (kinds: per-site byte of scasml_plan_site_kinds
        or None; order: device int32 list of the sites to evaluate, in launch order -- the as-coded matrix-core kernel then launches over those
        sites only; f16_rows: the caller's rows were float16).  As coded: the matrix-core kernel where the rows may take fp16 planes
        (_fp16_planes) within their range, else the float64 kernel; the documented operators: the split demoted out of that range."""
        lib = _lib.load()
        self._require_trained()
        if self.compat is None:
            model = self._device_model(x_bound)
            if kinds is None:
                _lib.check(lib.scasml_gp_eval(C.byref(model), _lib.ptr(pts), n_rows, _lib.ptr(out4), None, _lib.stream_ptr()), "gp_eval")
            else:
                _lib.check(lib.scasml_gp_eval_sites(C.byref(model), _lib.ptr(pts), n_rows, rows_per_site, _lib.ptr(kinds),
                                                    _lib.ptr(out4), _lib.stream_ptr()), "gp_eval")
            return
        r16 = int(self.eval_round16)
        if self._fp16_planes(f16_rows) and self._compat_model is not None and self._fp16_in_range(x_bound):
            args = (_lib.ptr(self._compat_model), self.N_domain, self.N_boundary, self._idx_ptr, r16, float(x_bound), _lib.ptr(pts), n_rows)
            if order is not None and kinds is not None and rows_per_site % 32 == 0 and n_rows % rows_per_site == 0:
                name, args = "gp_eval_compat_site_list", args + (rows_per_site, _lib.ptr(kinds), _lib.ptr(order), int(order.numel()))
            else:
                name, args = "gp_eval_compat_sites", args + (rows_per_site if kinds is not None else 0, _lib.ptr(kinds))
        else:                 # the float64 kernel: no one-plane mode; the reference's float16 op sequence on f16_graph rows
            r16 &= _lib.ROUND16_ENTRIES | _lib.ROUND16_OUTPUTS
            if self._f16_graph_rows(f16_rows):
                r16 |= _lib.ROUND16_F16_OPS | self._f16_extra
            name, args = "gp_eval_compat", self._f64_model() + (r16, _lib.ptr(pts), n_rows, pts.shape[1])
        head = (self.d, self.a, float(self.equation.sigma()), float(self.equation.mu()), int(self.equation.eq_id))
        _lib.check(getattr(lib, "scasml_" + name)(*head, *args, _lib.ptr(out4), None, _lib.stream_ptr()), name)

    def _predict_device(self, x_dev):
        pts, _, hb, f16 = self._points_device(x_dev)
        return self._eval_device(pts, hb, f16)[:, 0:1]

    # ------------------------------------------------------------------ training
    def _set_collocation(self, x_t_domain, x_t_boundary):
        """Take the collocation sets: host copies, new float32 device tensors (a cached factor belongs to THESE tensors, _L_made_for), sizes."""
        torch = _lib.require_gpu()
        self.x_t_domain, self.x_t_boundary = np.asarray(x_t_domain), np.asarray(x_t_boundary)
        self._xd = torch.from_numpy(np.ascontiguousarray(self.x_t_domain, dtype=np.float32)).cuda()
        self._xb = torch.from_numpy(np.ascontiguousarray(self.x_t_boundary, dtype=np.float32)).cuda()
        self.N_domain, self.N_boundary = self._xd.shape[0], self._xb.shape[0]
        self.phi_dim = 4 * self.N_domain + self.N_boundary

    @staticmethod
    def _identity_padded(A):
        """A copy of the square device matrix A in the top left of an identity, its order rounded up to 32 (what the blocked FP64 kernels take)."""
        torch = _lib.require_gpu()
        n = A.shape[0]
        Ap = torch.eye(_round_up(n, 32), dtype=torch.float64, device="cuda")
        Ap[:n, :n] = A
        return Ap

    def _factor(self, Ap, nugget, what, stage=None):
        """Cholesky of Ap + nugget I in place (Ap identity-padded, lower triangle read); returns the pivot info, 0 when positive definite.
        stage: the name under which kernel_phi_phi has the call timed."""
        torch = _lib.require_gpu()
        info = torch.zeros(1, dtype=torch.int32, device="cuda")
        call = lambda: _lib.check(_lib.load().scasml_cholesky(_lib.ptr(Ap), Ap.shape[0], float(nugget), _lib.ptr(info), _lib.stream_ptr()), what)
        if stage:
            self._stage(stage, call)
        else:
            call()
        return int(info.item())

    def _factor_padded(self, A, nugget, what, stage=None):
        """(factor, pivot info) of A + nugget I, factored in an identity-padded copy of A."""
        Ap = self._identity_padded(A)
        return Ap, self._factor(Ap, nugget, what, stage)

    def kernel_phi_phi(self, x_t_domain, x_t_boundary):
        '''K(phi,phi) + nugget*I as a CUDA float64 tensor; also factors it (models/GP.py:182-268).'''
        torch = _lib.require_gpu()
        lib = _lib.load()
        self._set_collocation(x_t_domain, x_t_boundary)
        xd, xb, M = self._xd, self._xb, self.phi_dim
        s = _lib.stream_ptr()
        K = torch.empty((M, M), dtype=torch.float64, device="cuda")
        as_coded = self.compat == "reference"
        name = "gp_gram_compat" if as_coded else "gp_gram"
        compat_args = (self._idx_ptr, self._gram_bits(xd, xb)) if as_coded else ()
        self._stage("gram", lambda: _lib.check(getattr(lib, "scasml_" + name)(
            self.d, self.a, _lib.ptr(xd), self.N_domain, _lib.ptr(xb), self.N_boundary, *compat_args, _lib.ptr(K), s), name))
        L, info = self._factor_padded(K, self.nugget, "cholesky", stage="cholesky")
        if info != 0 or bool(torch.isnan(L).any()):
            raise ValueError("Cholesky decomposition resulted in NaN values.")        # models/GP.py:264-265
        self._L_pad = L
        self._L_made_for = (xd, xb, self.nugget, self.sigma)   # predict_variance: the factor belongs to these collocation tensors, this noise and scale
        self.cholesky_phi_phi_perturb = L[:M, :M]
        if as_coded:                       # kernel_phi_phi_perturb.astype(float16) (:268): the entries are float16 already, the diagonal moves
            _lib.check(lib.scasml_round16_diag(_lib.ptr(K), M, M, float(self.nugget), s), "round16_diag")
        else:
            K.diagonal().add_(self.nugget)
        return K

    def rhs_f(self, x_t_domain):
        raise NotImplementedError

    def bdy_g(self, x_t_boundary):
        xb = np.asarray(x_t_boundary)
        if self.compat == "reference" and _f16_exact(xb):
            xb = xb.astype(np.float16)      # the reference's boundary points are float16 arrays: g is then its float16 graph (equations.py:259-261)
        else:
            xb = xb.astype(np.float64)      # the documented operators: no float16 emulation anywhere
        return np.asarray(self.equation.g(xb), dtype=np.float64)[:, 0]   # models/GP.py:417-419

    def time_der_rep(self, sol, rhs_f):
        raise NotImplementedError

    def loss_function(self, sol, rhs_f=None, bdy_g=None, L=None):
        '''The Newton objective |L^-1 b(sol)|^2 with b = [z1, g(x_bdy), z3, F(sol) + rhs_f, z5] (models/GP.py:430-444), on the device: b by
        scasml_gp_newton_b, one blocked triangular solve against the factor of kernel_phi_phi.  ``L`` (optional): another factor of the same order.
        The reference solves ``jnp.linalg.solve(L, b)`` with its own factor, the DENSE U sqrt(S + nugget) of the SVD (:260-266, 439): a factor that
        is not lower triangular is therefore accepted too -- |L^-1 b|^2 = b^T (L L^T)^-1 b, evaluated through the Cholesky factor of L L^T (the
        triangular solve reads the lower triangle only and would silently ignore the rest).  Returns a float64 scalar (the reference casts the
        value to float16 for its log).'''
        torch = _lib.require_gpu()
        lib = _lib.load()
        if getattr(self, "N_domain", None) is None or getattr(self, "x_t_boundary", None) is None:
            raise _lib.ScasmlError("no collocation points: call kernel_phi_phi(x_domain, x_boundary) or GPsolver first (N_domain and x_t_boundary are set there)")
        if getattr(self, "_L_pad", None) is None and L is None:
            raise _lib.ScasmlError("no factor: call kernel_phi_phi(x_domain, x_boundary) or GPsolver first")
        N, Nb, M = self.N_domain, self.N_boundary, self.phi_dim
        s = _lib.stream_ptr()
        sol_d = torch.as_tensor(np.asarray(sol, dtype=np.float64).reshape(-1), device="cuda").contiguous()
        if sol_d.numel() != 3 * N:
            raise ValueError("sol has %d entries, expected 3 N_domain = %d" % (sol_d.numel(), 3 * N))
        g = self.bdy_g(self.x_t_boundary) if bdy_g is None else np.asarray(bdy_g, dtype=np.float64).reshape(-1)
        g_d = torch.as_tensor(np.asarray(g, dtype=np.float64), device="cuda").contiguous()
        if L is None:
            Lp = self._L_pad
        else:
            Lg = torch.as_tensor(np.asarray(L.detach().cpu() if isinstance(L, torch.Tensor) else L, dtype=np.float64), device="cuda")
            if Lg.shape != (M, M):
                raise ValueError("L has shape %s, expected (%d, %d)" % (tuple(Lg.shape), M, M))
            if bool((torch.triu(Lg, 1) != 0).any()):          # a general factor (the reference's own is U sqrt(S)): the Cholesky factor of L L^T
                Lp, info = self._factor_padded(Lg @ Lg.T, 0.0, "cholesky(L L^T)")
                if info != 0:
                    raise ValueError("L L^T is not positive definite")
            else:
                Lp = self._identity_padded(Lg)
        Mp = Lp.shape[0]
        b = torch.zeros((Mp, 1), dtype=torch.float64, device="cuda")
        _lib.check(lib.scasml_gp_newton_b(int(self.equation.eq_id), int(self.d), float(self.equation.sigma()), float(self.equation.mu()), _lib.ptr(sol_d),
                                          _lib.ptr(g_d), N, Nb, _lib.ptr(b), s), "gp_newton_b")
        if rhs_f is not None:
            b[2 * N + Nb:3 * N + Nb, 0] += torch.as_tensor(np.asarray(rhs_f, dtype=np.float64).reshape(-1), device="cuda")
        _lib.check(lib.scasml_trsm_lower(_lib.ptr(Lp), Mp, _lib.ptr(b), 1, 0, s), "trsm")
        return np.float64(torch.dot(b[:, 0], b[:, 0]).item())

    def _chol_solve_padded(self, Hp, rhs, n, damping):
        """(H + damping*I)^-1 rhs on an identity-padded system (in place Cholesky + two triangular solves); None if not SPD."""
        torch = _lib.require_gpu()
        lib = _lib.load()
        npad = Hp.shape[0]
        s = _lib.stream_ptr()
        if self._factor(Hp, damping, "cholesky(newton)") != 0:
            return None
        b = torch.zeros((npad, 1), dtype=torch.float64, device="cuda")
        b[:n, 0] = rhs
        _lib.check(lib.scasml_trsm_lower(_lib.ptr(Hp), npad, _lib.ptr(b), 1, 0, s), "trsm")
        _lib.check(lib.scasml_trsm_lower(_lib.ptr(Hp), npad, _lib.ptr(b), 1, 1, s), "trsm^T")
        return b[:n, 0]

    def GPsolver(self, x_t_domain, x_t_boundary, GN_steps=20):
        '''Newton's method on b(sol)^T K_p^-1 b(sol) (models/GP.py:487-604); returns predict(x_domain).

        Host code only sequences kernels and reads two scalars per step (loss, gradient norm): Gram, Cholesky,
        K_p^-1 (two blocked triangular solves on the identity), b(sol), A b, gradient + Hessian assembly and the
        Newton solve all run in libscasml_hip (scasml_gp_gram / _cholesky / _trsm_lower / _gp_newton_b / _gemv /
        _gp_newton_system).'''
        torch = _lib.require_gpu()
        lib = _lib.load()
        if getattr(self.equation, "eq_id", None) is None or getattr(self.equation, "surrogate_free_only", False):
            raise NotImplementedError("no HIP Newton kernels for equation %s%s" % (type(self.equation).__name__, " (its f depends on |z|^2: the collocation operator of "
                                      "models/GP.py:705-719 is a function of (u, Lap u, div u) alone)" if getattr(self.equation, "eq_id", None) is not None else ""))
        Kp = self.kernel_phi_phi(x_t_domain, x_t_boundary)
        if self.compat != "reference":
            del Kp
        N, Nb, M = self.N_domain, self.N_boundary, self.phi_dim
        L = self._L_pad
        Mp = L.shape[0]
        s = _lib.stream_ptr()
        eq_id, d, sig, mu = int(self.equation.eq_id), int(self.d), float(self.equation.sigma()), float(self.equation.mu())
        A = torch.empty((Mp, Mp), dtype=torch.float64, device="cuda")   # -> K_p^-1 = L^-T L^-1
        self._stage("inverse", lambda: _lib.check(lib.scasml_cholesky_inverse(_lib.ptr(L), Mp, _lib.ptr(A), s), "cholesky_inverse"))
        bdy_g = torch.as_tensor(np.asarray(self.bdy_g(self.x_t_boundary), dtype=np.float64), device="cuda").contiguous()
        sol = torch.zeros(3 * N, dtype=torch.float64, device="cuda")
        b = torch.empty(M, dtype=torch.float64, device="cuda")
        Ab = torch.empty(M, dtype=torch.float64, device="cuda")
        grad = torch.empty(3 * N, dtype=torch.float64, device="cuda")
        npad = _round_up(3 * N, 32)
        H = torch.empty((npad, npad), dtype=torch.float64, device="cuda")
        damping = 1e-4                                                  # models/GP.py:490

        def residual(sol_):
            _lib.check(lib.scasml_gp_newton_b(eq_id, d, sig, mu, _lib.ptr(sol_), _lib.ptr(bdy_g), N, Nb, _lib.ptr(b), s), "gp_newton_b")
            _lib.check(lib.scasml_gemv(_lib.ptr(A), M, Mp, _lib.ptr(b), _lib.ptr(Ab), s), "gemv")
            return float(torch.dot(b, Ab))                              # loss = b^T A b, :430-444

        hist = [residual(sol)]
        self.grad_norms = []                                            # ||grad J|| at the start of every iteration (:518-519)
        for _ in range(GN_steps):                                       # :515-588
            _lib.check(lib.scasml_gp_newton_system(eq_id, d, sig, mu, _lib.ptr(A), Mp, N, Nb, _lib.ptr(sol), _lib.ptr(Ab),
                                                   _lib.ptr(grad), _lib.ptr(H), npad, 0, s), "gp_newton_system")
            self.grad_norms.append(float(torch.linalg.vector_norm(grad)))
            if self.grad_norms[-1] < 1e-5:                              # :521
                break
            step = self._chol_solve_padded(H, -grad, 3 * N, damping)   # :529-533 (H is overwritten by its factor)
            if step is None:
                # the full Hessian (:511) is indefinite at this iterate (large collocation sets): the reference's LU
                # solve would take the step regardless; use the Gauss-Newton part, which is positive semidefinite
                self.gauss_newton_steps = getattr(self, "gauss_newton_steps", 0) + 1
                _lib.check(lib.scasml_gp_newton_system(eq_id, d, sig, mu, _lib.ptr(A), Mp, N, Nb, _lib.ptr(sol), _lib.ptr(Ab),
                                                       _lib.ptr(grad), _lib.ptr(H), npad, 1, s), "gp_newton_system(GN)")
                step = self._chol_solve_padded(H, -grad, 3 * N, damping)
            if step is None:
                raise ValueError("Newton system is not positive definite")
            sol = sol + step                                            # alpha = 1, :541,573
            hist.append(residual(sol))
        self.loss_history = hist
        if self.compat == "reference":
            # z4 = time_der_rep(sol).astype(float16) (:719), right_vector = solve(float16(K_p), z) (:268, 599): a second
            # factorisation, of the rounded matrix (still positive definite: rounding moves only the diagonal, by < nugget)
            _lib.check(lib.scasml_round16(C.c_void_p(b.data_ptr() + 8 * (2 * N + Nb)), N, s), "round16")
            Lp = self._identity_padded(Kp)
            del Kp
            rv = self._chol_solve_padded(Lp, b, M, 0.0)
            del Lp
            if rv is None:
                raise ValueError("float16-rounded K_p is not positive definite")
            rv = rv.contiguous()
        else:
            rv = torch.empty(M, dtype=torch.float64, device="cuda")
            _lib.check(lib.scasml_gemv(_lib.ptr(A), M, Mp, _lib.ptr(b), _lib.ptr(rv), s), "gemv")   # right_vector = K_p^-1 z, :593-600
        self.right_vector = rv.cpu().numpy()[:, None]
        self._sol = sol
        self._pack(rv)
        return self.predict(x_t_domain)                                 # :602

    def _pack(self, rv):
        torch = _lib.require_gpu()
        lib = _lib.load()
        N = self.N_domain + self.N_boundary
        self._n_pad = _round_up(N, _lib.GP_TILE)
        # collocation points that are exactly float16 (the reference's deepxde float16 arrays are) need one plane, and are what the
        # matrix-core form of the as-coded surrogate needs
        self._colloc_is_f16 = _f16_exact(self._xd, self._xb)
        if self.compat == "reference":
            self._colloc_t = torch.empty((self.d + 1, N), dtype=torch.float64, device="cuda")
            _lib.check(lib.scasml_gp_compat_pack(self.d, _lib.ptr(self._xd), self.N_domain, _lib.ptr(self._xb), self.N_boundary,
                                                 _lib.ptr(self._colloc_t), N, _lib.stream_ptr()), "gp_compat_pack")
            self._rv_dev = rv.to(dtype=torch.float64).contiguous().clone()
            self._compat_model = None
            if self._colloc_is_f16:
                self._compat_model = torch.empty((int(lib.scasml_gp_compat_model_floats(self.d, self._n_pad)),), dtype=torch.float32, device="cuda")
                _lib.check(lib.scasml_gp_compat_pack_mfma(self.d, self.a, _lib.ptr(self._xd), self.N_domain, _lib.ptr(self._xb),
                                                          self.N_boundary, _lib.ptr(self._rv_dev), self._idx_ptr, _lib.ptr(self._compat_model),
                                                          _lib.stream_ptr()), "gp_compat_pack_mfma")
        else:
            kp = int(lib.scasml_point_stride(self.d))
            self._colloc = torch.empty((self._n_pad, kp), dtype=torch.float32, device="cuda")
            self._frag = torch.empty((self._n_pad * kp,), dtype=torch.float32, device="cuda")
            self._bf16 = torch.empty((int(lib.scasml_gp_plane_halfwords(self.d, self._n_pad)),), dtype=torch.int16, device="cuda")
            self._coef = torch.empty((int(lib.scasml_gp_coef_floats(self._n_pad)),), dtype=torch.float32, device="cuda")
            rv = rv.contiguous()
            _lib.check(lib.scasml_gp_pack(self.d, self.a, float(self.T), _lib.ptr(self._xd), self.N_domain,
                                          _lib.ptr(self._xb), self.N_boundary, _lib.ptr(rv), _lib.ptr(self._colloc),
                                          _lib.ptr(self._frag), _lib.ptr(self._bf16), _lib.ptr(self._coef), _lib.stream_ptr()), "gp_pack")
        torch.cuda.current_stream().synchronize()                  # rv may be freed by the caller

    def load_right_vector(self, x_t_domain, x_t_boundary, right_vector):
        '''Install a trained state (collocation points + right_vector) without running GPsolver.'''
        torch = _lib.require_gpu()
        self._set_collocation(x_t_domain, x_t_boundary)
        rv = np.asarray(right_vector, dtype=np.float64).reshape(-1)
        if rv.size != self.phi_dim:
            raise ValueError("right_vector has %d entries, expected %d" % (rv.size, self.phi_dim))
        self.right_vector = rv[:, None]
        self._pack(torch.from_numpy(rv).cuda())

    # ------------------------------------------------------------------ checkpoint / resume
    def state_dict(self):
        '''Everything inference needs, as NumPy arrays: collocation points, right_vector, loss history.'''
        if self.right_vector is None:
            raise _lib.ScasmlError("GP is not trained: nothing to save")
        return {"n_input": np.int64(self.n_input), "x_t_domain": np.asarray(self.x_t_domain),
                "x_t_boundary": np.asarray(self.x_t_boundary), "right_vector": np.asarray(self.right_vector),
                "loss_history": np.asarray(getattr(self, "loss_history", []), dtype=np.float64),
                "nugget": np.float64(self.nugget), "sigma": np.float64(self.sigma), "T": np.float64(self.T), "compat": np.str_(self.compat or ""), "f16_graph": np.bool_(self.f16_graph),
                # the float16 op sequence is only taken on float16 collocation points; otherwise the fit silently used one rounding per entry
                "f16_graph_effective": np.bool_(self._f16_graph_rows(True)),
                "laplacian_idx": np.asarray(self.laplacian_idx if self.laplacian_idx is not None else [], dtype=np.int32)}

    def load_state_dict(self, state):
        if int(state["n_input"]) != self.n_input:
            raise ValueError("state is for n_input=%d, this GP has n_input=%d" % (int(state["n_input"]), self.n_input))
        if str(state.get("compat", "")) != (self.compat or "") or (
                self.compat and not np.array_equal(np.asarray(state["laplacian_idx"]), self.laplacian_idx)):
            trained = str(state.get("compat", ""))
            raise ValueError("state was trained with compat=%r, laplacian_idx=%s: construct the GP with compat=%s%s to load it" % (
                trained, state.get("laplacian_idx"), repr(trained) if trained else "None",
                (", laplacian_idx=%s" % np.asarray(state["laplacian_idx"]).tolist()) if trained else ""))
        if bool(state.get("f16_graph", False)) != bool(self.f16_graph):
            raise ValueError("state was trained with f16_graph=%s: construct the GP with the same flag" % bool(state.get("f16_graph", False)))
        self.nugget = float(state["nugget"])
        if "sigma" in state:                                # states saved before the scale was carried keep this object's value
            self.sigma = float(state["sigma"])
        if "T" in state and float(state["T"]) != float(self.T):
            raise ValueError("state was trained with terminal time T = %g, this GP's equation has T = %g" % (float(state["T"]), float(self.T)))
        self.loss_history = list(np.asarray(state["loss_history"], dtype=np.float64))
        self._sol = None                                    # the Newton unknowns of an earlier GPsolver do not belong to the loaded state
        self.load_right_vector(state["x_t_domain"], state["x_t_boundary"], state["right_vector"])
        return self

    def save(self, path):
        np.savez_compressed(path, **self.state_dict())

    def load(self, path):
        with np.load(path) as f:
            return self.load_state_dict({k: f[k] for k in f.files})

    # ------------------------------------------------------------------ inference
    def predict(self, x_t_infer):
        '''(n, 1) posterior mean (models/GP.py:653-671).'''
        pts, was_numpy, hb, f16 = self._points_device(x_t_infer)
        out = self._eval_device(pts, hb, f16)[:, 0:1]
        return out.cpu().numpy() if was_numpy else out

    # posterior variance (no counterpart in models/GP.py, which keeps only right_vector): var(x) = kappa(x, x) - |L^-1 K(x, phi)|^2 with the factor
    # L of K(phi, phi) + nugget I that kernel_phi_phi leaves on the device
    variance_buffer_bytes = 1 << 30     # cap of the (points x Mp) float64 row buffer predict_variance works in; n is walked in chunks under it
    cross_rows_per_call = 65535 * 16    # the most rows scasml_gp_cross_rows takes in one call; _cross_rows walks longer sets under it

    def _variance_factor(self):
        """The padded float64 factor of K(phi, phi) + nugget I for the collocation points this GP holds.  kernel_phi_phi / GPsolver leave it;
        after load_state_dict / load / load_right_vector it is rebuilt here, once, by kernel_phi_phi's own device work (Gram + Cholesky, same nugget)."""
        if getattr(self, "_xd", None) is None:
            raise _lib.ScasmlError("no collocation points yet: call GPsolver / kernel_phi_phi / load_right_vector first")
        made_for = getattr(self, "_L_made_for", None)
        if (getattr(self, "_L_pad", None) is None or made_for is None or made_for[0] is not self._xd or made_for[1] is not self._xb
                or made_for[2] != self.nugget or made_for[3] != self.sigma):
            self.kernel_phi_phi(self.x_t_domain, self.x_t_boundary)
        return self._L_pad

    def predict_variance(self, x_t_infer):
        '''(n, 1) float64 posterior variance  var(x) = kappa(x, x) - |L^-1 K(x, phi)|^2,  kappa(x, x) = 1  (NumPy in, NumPy out; CUDA tensor in, CUDA
        tensor out; the raw value, not clamped).

        compat=None: the posterior variance of u(x) under the prior kappa given noisy observations (noise variance = nugget) of the collocation
        functionals [u(dom), u(bdy), Lap(dom), dt(dom), div(dom)]; it lies in [0, 1] up to rounding.  compat="reference": the as-coded ANALOGUE --
        the same formula on the matrices the reference's code builds (float16-valued entries, 5-index Hutchinson Laplacian blocks on the shifted
        argument, lower triangle of K); those are not the Gram matrix and cross-covariances of one kernel, so the value carries no sign guarantee.
        It depends on the collocation points, sigma and nugget only -- not on the fit: kernel_phi_phi(x_dom, x_bdy) is enough, also for equations
        GPsolver has no Newton kernels for.

        The feature rows (scasml_gp_cross_rows, op 0) are written straight into a padded (points x Mp) float64 buffer and solved in place by
        scasml_gp_variance (one FP64-MFMA launch per chunk, the sums of squares in the same kernel); n is walked in chunks that keep the buffer
        under ``variance_buffer_bytes``.  Every point's value is a function of that point alone, bit for bit: chunking and order do not change it.
        Needs the factor of K(phi, phi) + nugget I: GPsolver / kernel_phi_phi leave it; after load_state_dict / load / load_right_vector the first
        call rebuilds it (one Gram + one Cholesky factorisation) and keeps it.  state_dict does not carry it.'''
        torch = _lib.require_gpu()
        L = self._variance_factor()
        xi, was_numpy, f16_rows = self._rows_device(x_t_infer)
        n, Mp = xi.shape[0], L.shape[0]
        r16 = self._gram_bits(self._xd, self._xb, f16_rows)
        var = torch.empty((n, 1), dtype=torch.float64, device="cuda")
        chunk = int(max(1, min(self.variance_buffer_bytes // (8 * Mp), n)))
        rows = torch.zeros((chunk, Mp), dtype=torch.float64, device="cuda") if n else None
        for lo in range(0, n, chunk):
            self._solved_rows(L, xi[lo:lo + chunk], r16, rows, var[lo:])
        return var.cpu().numpy() if was_numpy else var

    def predict_std(self, x_t_infer):
        '''(n, 1) float64 posterior standard deviation sqrt(max(predict_variance, 0)).'''
        var = self.predict_variance(x_t_infer)
        return np.sqrt(np.maximum(var, 0.0)) if isinstance(var, np.ndarray) else var.clamp_min(0.0).sqrt()

    # posterior covariance of the four functionals at a point and the delta-method variance of the PDE residual (no counterpart in models/GP.py)
    def _functional_prior(self):
        """(4, 4) float64: the prior covariance of [u, Lap u, dt u, div u] at one point -- the Gram table (csrc/gp_gram_table.hpp) at r = 0."""
        a, d = self.a, float(self.d)
        P = np.zeros((4, 4), dtype=np.float64)
        P[0, 0] = 1.0
        P[0, 1] = P[1, 0] = -a * d
        P[1, 1] = (d * d + 2.0 * d) * a * a
        P[2, 2] = a
        P[3, 3] = a * d
        return P

    def _functional_covariance(self, xi, neg=None):
        """((n, 4, 4) covariance, (n, 4) means or None) on the device for the float32 device rows xi.  The four operators' feature rows go into one
        zeroed (chunk, 4, Mp) buffer -- operator o at column offset o Mp of a row of 4 Mp doubles, so the rows lie interleaved without a copy -- and
        scasml_gp_functional_covariance solves them in place.  neg, (1, Mp) = -right_vector padded with zeros: the posterior-mean functionals
        K_o(x, phi) . right_vector are taken from the same buffer before it is solved (scasml_gemm_nt_sub, one column)."""
        torch = _lib.require_gpu()
        lib = _lib.load()
        L = self._variance_factor()
        n, Mp = xi.shape[0], L.shape[0]
        f64 = dict(dtype=torch.float64, device="cuda")
        cov = torch.empty((n, 4, 4), **f64)
        mean = torch.zeros((n, 4), **f64) if neg is not None else None
        if n == 0:
            return cov, mean
        prior = np.ascontiguousarray(self._functional_prior())
        chunk = int(max(1, min(self.variance_buffer_bytes // (32 * Mp), self.cross_rows_per_call, n)))
        buf = torch.zeros((chunk, 4, Mp), **f64)             # columns M .. Mp stay zero through every solve: L is the identity there
        for lo in range(0, n, chunk):
            xc = xi[lo:lo + chunk]
            c = xc.shape[0]
            for o in range(4):
                self._cross_rows(self._xd, self._xb, o, xc, buf[:, o, :], 4 * Mp, 0)
            if neg is not None:
                self._gemm_nt_sub(mean[lo:lo + c].view(4 * c, 1), buf, Mp, neg, Mp)
            _lib.check(lib.scasml_gp_functional_covariance(_lib.ptr(L), Mp, _lib.ptr(buf), Mp, c, prior.ctypes.data_as(C.c_void_p), _lib.ptr(cov[lo:]),
                                                           _lib.stream_ptr()), "gp_functional_covariance")
        return cov, mean

    def predict_functional_covariance(self, x_t_infer):
        '''(n, 4, 4) float64 posterior covariance of [u, Lap u, dt u, div u] at each point (NumPy in, NumPy out; CUDA tensor in, CUDA tensor out; the
        raw values, not clamped):
            cov(x)[o][p] = P[o][p] - (L^-1 K_o(x, phi)) . (L^-1 K_p(x, phi))
        with P the prior covariance of the four functionals at one point (1, -a d, (d^2 + 2 d) a^2, a, a d: the Gram table at r = 0), K_o the op-o
        feature rows of scasml_gp_cross_rows and L the factor predict_variance uses.  One launch of scasml_gp_functional_covariance per chunk
        (csrc/gp_functional_cov.hip): n is walked in chunks that keep the (points x 4 x Mp) row buffer under ``variance_buffer_bytes``.  Every point's
        block is a function of that point alone, bit for bit; it is exactly symmetric, and [:, 0, 0] is predict_variance bit for bit.  It depends on
        the collocation points, sigma and nugget only -- not on the fit.  compat=None only.'''
        if self.compat == "reference":
            raise ValueError("the functional covariance needs compat=None: the as-coded matrix is not the Gram of one kernel and has no derivative in a")
        xi, was_numpy, _ = self._rows_device(x_t_infer)
        cov = self._functional_covariance(xi)[0]
        return cov.cpu().numpy() if was_numpy else cov

    def predict_residual_variance(self, x_t_infer, return_parts=False):
        '''(n, 1) float64 delta-method variance  c^T cov c  of the PDE residual  r = dt u - F(u, Lap u, div u)  at each point (NumPy in, NumPy out; CUDA
        tensor in, CUDA tensor out; the raw value, not clamped), cov = predict_functional_covariance(x) and
            c = [-dF/dz1, -dF/dz3, 1, -dF/dz5]   (equation.F_parts)
        evaluated at the float64 posterior-mean functionals m_o(x) = K_o(x, phi) . right_vector, which are taken from the covariance's own row buffer
        before it is solved.  F_parts is host NumPy; the 4 x 4 combine is elementwise, one fixed order: a point's value is a function of that point
        alone, bit for bit.  return_parts=True: (variance, {"mean": (n, 4) m, "c": (n, 4), "residual": (n, 1) m_dt - F(m)}).  Needs a trained GP and
        an equation with F_parts (NotImplementedError otherwise); compat=None only.'''
        torch = _lib.require_gpu()
        if self.compat == "reference":
            raise ValueError("the residual variance needs compat=None: the as-coded matrix is not the Gram of one kernel and has no derivative in a")
        if self.right_vector is None:
            raise NotImplementedError("the residual variance is linearised at the posterior mean: call GPsolver(x_domain, x_boundary) first")
        if not callable(getattr(self.equation, "F_parts", None)):
            raise NotImplementedError("the residual variance needs the equation's collocation operator and its derivatives: %s has no F_parts"
                                      % type(self.equation).__name__)
        xi, was_numpy, _ = self._rows_device(x_t_infer)
        n = xi.shape[0]
        neg = torch.zeros((1, _round_up(self.phi_dim, 32)), dtype=torch.float64, device="cuda")
        neg[0, :self.phi_dim] = -torch.from_numpy(np.ascontiguousarray(self.right_vector, dtype=np.float64).reshape(-1)).cuda()
        cov, mean = self._functional_covariance(xi, neg)
        m = mean.cpu().numpy()
        F, (d1, d3, d5) = self.equation.F_parts(m[:, 0], m[:, 1], m[:, 3])[:2]
        c_h = np.stack([-np.broadcast_to(d1, (n,)), -np.broadcast_to(d3, (n,)), np.ones(n), -np.broadcast_to(d5, (n,))], axis=1).astype(np.float64)
        c = torch.from_numpy(np.ascontiguousarray(c_h)).cuda()
        var = torch.zeros((n, 1), dtype=torch.float64, device="cuda")
        for o in range(4):                                   # sum_o c_o (sum_p cov[o][p] c_p), p then o rising
            inner = torch.zeros(n, dtype=torch.float64, device="cuda")
            for p in range(4):
                inner.addcmul_(cov[:, o, p], c[:, p])
            var[:, 0].addcmul_(c[:, o], inner)
        if not return_parts:
            return var.cpu().numpy() if was_numpy else var
        res_h = (m[:, 2] - np.asarray(F, dtype=np.float64))[:, None]
        parts = {"mean": m, "c": c_h, "residual": res_h} if was_numpy else {"mean": mean, "c": c, "residual": torch.from_numpy(res_h).cuda()}
        return (var.cpu().numpy() if was_numpy else var), parts

    def predict_residual_std(self, x_t_infer):
        '''(n, 1) float64 sqrt(max(predict_residual_variance, 0)).'''
        var = self.predict_residual_variance(x_t_infer)
        return np.sqrt(np.maximum(var, 0.0)) if isinstance(var, np.ndarray) else var.clamp_min(0.0).sqrt()

    # log marginal likelihood, its gradient and a fit of (sigma, nugget) to it (no counterpart in models/GP.py, which hard-codes both, :25-26)
    def _evidence_ready(self):
        if self.compat == "reference":
            raise ValueError("the log marginal likelihood needs compat=None: the as-coded matrix is not the Gram of one kernel and has no derivative in a")
        if getattr(self, "_xd", None) is None:
            raise _lib.ScasmlError("no collocation points yet: call GPsolver / kernel_phi_phi / load_right_vector first")

    def _gram_at(self, a):
        """K(a) of the documented operators on the held collocation points, (M, M) float64 on the device, nothing added to the diagonal."""
        torch = _lib.require_gpu()
        M = self.phi_dim
        K = torch.empty((M, M), dtype=torch.float64, device="cuda")
        _lib.check(_lib.load().scasml_gp_gram(self.d, float(a), _lib.ptr(self._xd), self.N_domain, _lib.ptr(self._xb), self.N_boundary, _lib.ptr(K),
                                              _lib.stream_ptr()), "gp_gram")
        return K

    def _evidence_z(self, z):
        """The M feature values the likelihood is taken of, float64 on the device: the caller's, else b(sol) of the fit, else K_p right_vector."""
        torch = _lib.require_gpu()
        lib = _lib.load()
        N, Nb, M = self.N_domain, self.N_boundary, self.phi_dim
        s = _lib.stream_ptr()
        if z is not None:
            zt = z.detach() if isinstance(z, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(np.asarray(z, dtype=np.float64)))
            zt = zt.to(device="cuda", dtype=torch.float64).reshape(-1).contiguous()
            if zt.numel() != M:
                raise ValueError("z has %d entries, expected 4 N_domain + N_boundary = %d" % (zt.numel(), M))
            return zt
        sol = getattr(self, "_sol", None)
        if sol is not None and sol.numel() == 3 * N:                   # b(sol) = [z1, g, z3, F(sol), z5], as GPsolver's last residual built it
            g = torch.as_tensor(np.asarray(self.bdy_g(self.x_t_boundary), dtype=np.float64), device="cuda").contiguous()
            b = torch.empty(M, dtype=torch.float64, device="cuda")
            _lib.check(lib.scasml_gp_newton_b(int(self.equation.eq_id), int(self.d), float(self.equation.sigma()), float(self.equation.mu()),
                                              _lib.ptr(sol.contiguous()), _lib.ptr(g), N, Nb, _lib.ptr(b), s), "gp_newton_b")
            return b
        if self.right_vector is None:
            raise _lib.ScasmlError("no feature values: pass z, or fit (GPsolver) or load a right_vector first")
        rv = torch.from_numpy(np.ascontiguousarray(np.asarray(self.right_vector, dtype=np.float64).reshape(-1))).cuda()
        K = self._gram_at(self.a)
        out = torch.empty(M, dtype=torch.float64, device="cuda")
        _lib.check(lib.scasml_gemv(_lib.ptr(K), M, M, _lib.ptr(rv), _lib.ptr(out), s), "gemv")
        return out.add_(rv, alpha=float(self.nugget))                  # z = K_p right_vector

    def _evidence_factor(self, sigma, nugget):
        """The padded factor of K(1 / sigma^2) + nugget I: the cached one at the object's own values, else a fresh one that is not kept (None when
        the matrix is not positive definite there).  A fresh one is kernel_phi_phi's own device work: the same bits a GP holding these values gets."""
        torch = _lib.require_gpu()
        if sigma == self.sigma and nugget == self.nugget:
            return self._variance_factor()
        L, info = self._factor_padded(self._gram_at(self._a_of(sigma)), nugget, "cholesky(evidence)")
        return None if info != 0 or bool(torch.isnan(L).any()) else L

    def _inverse_and_alpha(self, L, zt):
        """(A = K_p^-1 as an Mp x Mp device matrix, alpha = A z) from the padded factor L: what the gradients of the evidence and of the leave-one-out
        likelihood both start from."""
        torch = _lib.require_gpu()
        lib = _lib.load()
        M, Mp = self.phi_dim, L.shape[0]
        s = _lib.stream_ptr()
        A = torch.empty((Mp, Mp), dtype=torch.float64, device="cuda")
        _lib.check(lib.scasml_cholesky_inverse(_lib.ptr(L), Mp, _lib.ptr(A), s), "cholesky_inverse")
        alpha = torch.empty(M, dtype=torch.float64, device="cuda")
        _lib.check(lib.scasml_gemv(_lib.ptr(A), M, Mp, _lib.ptr(zt), _lib.ptr(alpha), s), "gemv")
        return A, alpha

    def _evidence(self, zt, sigma, nugget, return_grad):
        """(LML, (dLML/dlog sigma, dLML/dlog nugget) or None) at (sigma, nugget) for the device vector zt; None where K_p is not positive definite."""
        torch = _lib.require_gpu()
        lib = _lib.load()
        M = self.phi_dim
        s = _lib.stream_ptr()
        L = self._evidence_factor(sigma, nugget)
        if L is None:
            return None
        Mp = L.shape[0]
        y = torch.zeros((Mp, 1), dtype=torch.float64, device="cuda")
        y[:M, 0] = zt
        _lib.check(lib.scasml_trsm_lower(_lib.ptr(L), Mp, _lib.ptr(y), 1, 0, s), "trsm")           # y = L^-1 z:  z^T alpha = |y|^2
        out = torch.zeros(8, dtype=torch.float64, device="cuda")      # [log det, |y|^2, alpha^T K_a alpha, <A, K_a>, tr A, |alpha|^2]
        _lib.check(lib.scasml_chol_logdet(_lib.ptr(L), Mp, _lib.ptr(out), s), "chol_logdet")
        # the factor of the identity-padded K + nugget I has sqrt(1 + nugget), not 1, on its padding rows (scasml_cholesky adds the nugget to the
        # whole diagonal): their share of the sum is taken off again
        out[0] -= 2.0 * torch.log(L.diagonal()[M:]).sum()
        out[1] = torch.dot(y[:, 0], y[:, 0])
        if return_grad:
            a = self._a_of(sigma)
            A, alpha = self._inverse_and_alpha(L, zt)
            work = torch.empty(int(lib.scasml_gp_gram_da_contract_doubles(self.N_domain, self.N_boundary)), dtype=torch.float64, device="cuda")
            _lib.check(lib.scasml_gp_gram_da_contract(self.d, a, _lib.ptr(self._xd), self.N_domain, _lib.ptr(self._xb), self.N_boundary, _lib.ptr(A), Mp,
                                                      _lib.ptr(alpha), _lib.ptr(work), s), "gp_gram_da_contract")
            out[2:4] = work[:2]
            out[4] = A.diagonal()[:M].sum()
            out[5] = torch.dot(alpha, alpha)
        logdet, quad, q_a, t_a, tr_a, aa = out.cpu().numpy()[:6].tolist()
        value = -0.5 * quad - 0.5 * logdet - 0.5 * M * float(np.log(2.0 * np.pi))
        if not return_grad:
            return value, None
        d_a = 0.5 * q_a - 0.5 * t_a
        d_eta = 0.5 * aa - 0.5 * tr_a
        return value, (-2.0 * a * d_a, float(nugget) * d_eta)

    def log_marginal_likelihood(self, z=None, return_grad=False, sigma=None, nugget=None):
        '''log p(z | sigma, nugget) of the M = 4 N_domain + N_boundary feature values z under the documented-operator prior (compat=None only; the
        as-coded matrix is not the Gram of one kernel: ValueError), on the collocation points this object holds:

            LML = -1/2 z^T alpha - 1/2 log det K_p - M/2 log(2 pi),    K_p = K(a) + nugget I,  a = 1 / sigma^2,  alpha = K_p^-1 z.

        Returns a float; with return_grad=True ``(value, {"log_sigma": dLML/dlog sigma, "log_nugget": dLML/dlog nugget})``, where
        dLML/dlog sigma = -2 a dLML/da, dLML/da = 1/2 alpha^T K_a alpha - 1/2 tr(K_p^-1 K_a) with K_a = dK/da, and dLML/dlog nugget =
        nugget (1/2 alpha^T alpha - 1/2 tr K_p^-1).

        z: an array of M values; None: the fit's own feature vector b(sol) = [z1, g, z3, F(sol), z5] after GPsolver (rebuilt from the Newton unknowns
        by scasml_gp_newton_b), else K_p right_vector after load_state_dict / load_right_vector (the two agree to rounding).  sigma / nugget: evaluate
        at other hyperparameters without changing the object or its cached factor; at the object's own values the cached factor is reused.

        Cost.  Value: one Gram and one Cholesky (none with the cached factor), one triangular solve, scasml_chol_logdet.  Gradient, in addition:
        scasml_cholesky_inverse, one scasml_gemv, scasml_gp_gram_da_contract (one pass of Gram-tile size on the FP64 matrix cores, K_a never stored),
        a trace and a dot product.  The gradient holds TWO Mp x Mp float64 matrices on the device, the factor and K_p^-1 (Mp = M rounded up to 32).
        Every sum has a fixed order: two calls return the same bits.'''
        self._evidence_ready()
        sigma = self.sigma if sigma is None else float(sigma)
        nugget = self.nugget if nugget is None else float(nugget)
        if not (sigma > 0.0 and nugget > 0.0):
            raise ValueError("sigma and nugget must be positive")
        res = self._evidence(self._evidence_z(z), sigma, nugget, bool(return_grad))
        if res is None:
            raise ValueError("K(sigma = %g) + %g I is not positive definite in float64" % (sigma, nugget))
        value, grad = res
        return (value, {"log_sigma": grad[0], "log_nugget": grad[1]}) if return_grad else value

    def optimize_hyperparameters(self, z=None, which=("sigma", "nugget"), bounds=None, gtol=None, max_iter=50, objective="lml"):
        '''Maximise log_marginal_likelihood(z; sigma, nugget) at FIXED z over the log of the parameters named in ``which`` (type-II maximum likelihood).

        A bounded BFGS iteration on the host in at most two variables (_maximize_bounded; every evaluation is one device value + gradient).  bounds:
        {"sigma": (lo, hi), "nugget": (lo, hi)}; default sigma within a factor 8 of its current value, nugget in [1e-6, 1]; a start outside is moved
        onto the bound.  Stops when max |dLML/dlog theta| <= gtol (default 1e-4 M) over the variables not held at a bound by the gradient, or after
        max_iter iterations.

        When it converges it sets self.sigma and self.nugget, refactors, sets right_vector = K_p^-1 z and re-packs, so predict, predict_variance and
        the solvers see the new model at once -- for a linear problem this is the complete refit; for the nonlinear fit alternate
        GPsolver -> optimize_hyperparameters() -> GPsolver by hand.  When it does not, the object is left as it was.
        Returns {"sigma_start", "nugget_start", "lml_start", "sigma", "nugget", "lml", "grad": {"log_sigma", "log_nugget"}, "evaluations",
        "iterations", "converged"}: the best point found, installed or not.

        objective="loo" maximises loo_log_predictive instead (the sum of the leave-one-out predictive log densities; INTEGRATION.md says when to
        prefer it): the same iteration, bounds, stopping rule (on dLOO/dlog theta) and installation, and the same report with "objective": "loo" added
        and "loo_start" / "loo" in place of "lml_start" / "lml".'''
        torch = _lib.require_gpu()
        lib = _lib.load()
        if objective not in ("lml", "loo"):
            raise ValueError("objective must be 'lml' or 'loo'")
        evaluate = self._evidence if objective == "lml" else self._loo_objective
        self._evidence_ready()
        which = (which,) if isinstance(which, str) else tuple(which)
        if not which or len(set(which)) != len(which) or any(w not in ("sigma", "nugget") for w in which):
            raise ValueError("which must name 'sigma', 'nugget' or both")
        zt = self._evidence_z(z)
        M = self.phi_dim
        start = {"sigma": float(self.sigma), "nugget": float(self.nugget)}
        box = {"sigma": (start["sigma"] / 8.0, start["sigma"] * 8.0), "nugget": (1e-6, 1.0)}
        for k, (lo, hi) in (bounds or {}).items():
            if k not in box or not 0.0 < float(lo) <= float(hi):
                raise ValueError("bounds: {'sigma': (lo, hi), 'nugget': (lo, hi)} with 0 < lo <= hi")
            box[k] = (float(lo), float(hi))
        gtol = 1e-4 * M if gtol is None else float(gtol)
        lo = np.log([box[w][0] for w in which])
        hi = np.log([box[w][1] for w in which])

        def fun(x):
            p = dict(start)
            p.update({w: float(np.exp(v)) for w, v in zip(which, x)})
            res = evaluate(zt, p["sigma"], p["nugget"], True)
            if res is None:
                return None
            return res[0], np.array([res[1][0 if w == "sigma" else 1] for w in which])

        lml_start = evaluate(zt, start["sigma"], start["nugget"], False)
        x, val, grad, evals, iters, converged = _maximize_bounded(fun, np.log([start[w] for w in which]), lo, hi, gtol, int(max_iter))
        best = dict(start)
        best.update({w: float(np.exp(v)) for w, v in zip(which, x)})
        full = evaluate(zt, best["sigma"], best["nugget"], True)          # both derivatives at the returned point, held parameters included
        report = {"sigma_start": start["sigma"], "nugget_start": start["nugget"], "lml_start": None if lml_start is None else lml_start[0],
                  "sigma": best["sigma"], "nugget": best["nugget"], "lml": val, "grad": {"log_sigma": full[1][0], "log_nugget": full[1][1]},
                  "evaluations": evals + 2, "iterations": iters, "converged": bool(converged)}
        if objective == "loo":
            report = {("loo" + k[3:] if k.startswith("lml") else k): v for k, v in report.items()}
            report["objective"] = "loo"
        if not converged:
            return report
        self.sigma, self.nugget = best["sigma"], best["nugget"]
        L = self._variance_factor()                                     # refactors: the cache key holds both parameters
        Mp = L.shape[0]
        rv = torch.zeros((Mp, 1), dtype=torch.float64, device="cuda")
        rv[:M, 0] = zt
        s = _lib.stream_ptr()
        _lib.check(lib.scasml_trsm_lower(_lib.ptr(L), Mp, _lib.ptr(rv), 1, 0, s), "trsm")
        _lib.check(lib.scasml_trsm_lower(_lib.ptr(L), Mp, _lib.ptr(rv), 1, 1, s), "trsm^T")
        rv = rv[:M, 0].contiguous()
        self.right_vector = rv.cpu().numpy()[:, None]
        self._pack(rv)
        return report

    # leave-one-out cross-validation (Rasmussen & Williams 5.4.2; no counterpart in models/GP.py): what the other M - 1 collocation functionals
    # predict for each one, the sum of those predictive log densities and its gradient in (log sigma, log nugget)
    loo_panel_rows = 0      # rows of K_a per panel of scasml_gp_loo_da; 0: the library's default.  The result does not depend on it, bit for bit

    def _loo_blocks(self):
        N, Nb = self.N_domain, self.N_boundary
        edges = [0, N, N + Nb, 2 * N + Nb, 3 * N + Nb, 4 * N + Nb]
        return {name: slice(lo, hi) for name, lo, hi in zip(("u_dom", "u_bdy", "lap_dom", "dt_dom", "div_dom"), edges[:-1], edges[1:])}

    def _loo_state(self, zt, sigma, nugget):
        """(A = K_p^-1, alpha = A z, the diagonal of A over the M features) at (sigma, nugget); None where K_p is not positive definite."""
        L = self._evidence_factor(sigma, nugget)
        if L is None:
            return None
        A, alpha = self._inverse_and_alpha(L, zt)
        diag = A.diagonal()[:self.phi_dim].clone()
        if not bool((diag > 0.0).all()):              # also catches NaN
            return None
        return A, alpha, diag

    def _loo_objective(self, zt, sigma, nugget, return_grad):
        """(LOO, (dLOO/dlog sigma, dLOO/dlog nugget) or None) at (sigma, nugget) for the device vector zt; None where K_p is not positive definite.
        The signature of _evidence, so that optimize_hyperparameters feeds either to the same iteration."""
        torch = _lib.require_gpu()
        lib = _lib.load()
        state = self._loo_state(zt, sigma, nugget)
        if state is None:
            return None
        A, alpha, diag = state
        M, Mp = self.phi_dim, A.shape[0]
        s = _lib.stream_ptr()
        out = torch.zeros(3, dtype=torch.float64, device="cuda")      # [LOO, dLOO/da, dLOO/dnugget]
        out[0] = (0.5 * torch.log(diag) - alpha * alpha / (2.0 * diag) - 0.5 * float(np.log(2.0 * np.pi))).sum()
        if return_grad:
            a = self._a_of(sigma)
            q, v, Av, Aalpha = (torch.empty(M, dtype=torch.float64, device="cuda") for _ in range(4))
            work = torch.empty(int(lib.scasml_gp_loo_da_doubles(self.N_domain, self.N_boundary, int(self.loo_panel_rows))), dtype=torch.float64,
                               device="cuda")
            _lib.check(lib.scasml_gp_loo_da(self.d, a, _lib.ptr(self._xd), self.N_domain, _lib.ptr(self._xb), self.N_boundary, _lib.ptr(A), Mp,
                                            _lib.ptr(alpha), int(self.loo_panel_rows), _lib.ptr(q), _lib.ptr(v), _lib.ptr(work), s), "gp_loo_da")
            _lib.check(lib.scasml_gemv(_lib.ptr(A), M, Mp, _lib.ptr(v), _lib.ptr(Av), s), "gemv")              # (Z alpha) for theta = a
            _lib.check(lib.scasml_gemv(_lib.ptr(A), M, Mp, _lib.ptr(alpha), _lib.ptr(Aalpha), s), "gemv")      # (Z alpha) for theta = nugget
            ssq = torch.linalg.vector_norm(A[:M, :M], dim=1).square()      # s_i = sum_j A_ij^2: a row reduction of the view, no Mp^2 temporary
            w = 0.5 * (1.0 + alpha * alpha / diag)
            out[1] = ((alpha * Av - w * q) / diag).sum()
            out[2] = ((alpha * Aalpha - w * ssq) / diag).sum()
        value, d_a, d_eta = out.cpu().numpy().tolist()
        if not return_grad:
            return value, None
        return value, (-2.0 * a * d_a, float(nugget) * d_eta)

    def _loo_arguments(self, sigma, nugget):
        self._evidence_ready()
        sigma = self.sigma if sigma is None else float(sigma)
        nugget = self.nugget if nugget is None else float(nugget)
        if not (sigma > 0.0 and nugget > 0.0):
            raise ValueError("sigma and nugget must be positive")
        return sigma, nugget

    def loo(self, z=None, sigma=None, nugget=None):
        '''Leave-one-out diagnostics of the M = 4 N_domain + N_boundary collocation functionals (compat=None only, as log_marginal_likelihood): for
        each feature i, what the other M - 1 predict for it under K_p = K(a) + nugget I.  With A = K_p^-1 and alpha = A z

            mean_i = z_i - alpha_i / A_ii,   variance_i = 1 / A_ii,   residual_i = alpha_i / sqrt(A_ii) = (z_i - mean_i) / sqrt(variance_i),
            log_predictive_i = 1/2 log A_ii - alpha_i^2 / (2 A_ii) - 1/2 log(2 pi).

        Returns {"mean", "variance", "residual", "log_predictive": float64 NumPy arrays of M in the Gram's order [u(dom), u(bdy), Lap(dom), dt(dom),
        div(dom)], "blocks": {"u_dom", "u_bdy", "lap_dom", "dt_dom", "div_dom": the slice of each block}}.  z, sigma and nugget as in
        log_marginal_likelihood: overrides leave the object and its cached factor alone.  Cost: the factor (cached at the object's own values),
        scasml_cholesky_inverse, one scasml_gemv and element-wise work on M-vectors.'''
        torch = _lib.require_gpu()
        sigma, nugget = self._loo_arguments(sigma, nugget)
        zt = self._evidence_z(z)
        state = self._loo_state(zt, sigma, nugget)
        if state is None:
            raise ValueError("K(sigma = %g) + %g I is not positive definite in float64" % (sigma, nugget))
        _, alpha, diag = state
        res = {"mean": zt - alpha / diag, "variance": 1.0 / diag, "residual": alpha / torch.sqrt(diag),
               "log_predictive": 0.5 * torch.log(diag) - alpha * alpha / (2.0 * diag) - 0.5 * float(np.log(2.0 * np.pi))}
        res = {k: v.cpu().numpy() for k, v in res.items()}
        res["blocks"] = self._loo_blocks()
        return res

    def loo_log_predictive(self, z=None, return_grad=False, sigma=None, nugget=None):
        '''LOO = sum_i log p(z_i | z_-i, sigma, nugget), the leave-one-out predictive log-likelihood (the sum of loo()["log_predictive"]): the
        model-selection criterion that trusts the prior less than the evidence does.  Same arguments, defaults and refusals as
        log_marginal_likelihood; ValueError where K_p is not positive definite.

        Returns a float; with return_grad=True ``(value, {"log_sigma": dLOO/dlog sigma, "log_nugget": dLOO/dlog nugget})``, where for theta in
        (a, nugget), Z = A dK_p/dtheta,

            dLOO/dtheta = sum_i [ alpha_i (Z alpha)_i - 1/2 (1 + alpha_i^2 / A_ii) (Z A)_ii ] / A_ii,
            theta = a:       (Z alpha)_i = (A K_a alpha)_i,  (Z A)_ii = sum_jk A_ij K_a[j][k] A_ik;      dLOO/dlog sigma = -2 a dLOO/da
            theta = nugget:  (Z alpha)_i = (A alpha)_i,      (Z A)_ii = sum_j A_ij^2;                    dLOO/dlog nugget = nugget dLOO/dnugget.

        Cost of the gradient beyond loo(): scasml_gp_loo_da (the M^3 product A K_a A's diagonal on the FP64 matrix cores, K_a walked in row panels
        and never stored whole; workspace (panel rows + M / 64) M doubles), two scasml_gemv and a row reduction of A.  Every sum has a fixed order:
        two calls return the same bits.'''
        sigma, nugget = self._loo_arguments(sigma, nugget)
        res = self._loo_objective(self._evidence_z(z), sigma, nugget, bool(return_grad))
        if res is None:
            raise ValueError("K(sigma = %g) + %g I is not positive definite in float64" % (sigma, nugget))
        value, grad = res
        return (value, {"log_sigma": grad[0], "log_nugget": grad[1]}) if return_grad else value

    # joint posterior (no counterpart in models/GP.py): covariance between evaluation points and draws from N(mean, cov)
    def _cross_rows(self, x_dom, x_bdy, op, xi, out, ld, r16):
        """out[i] <- the operator-`op` feature row (op = 4: the gradient of the op-0 row) of every float32 device row xi[i] against the collocation
        sets (x_dom, x_bdy), the fitted ones or a caller's own: the one call of scasml_gp_cross_rows.  x_bdy may be empty; ld: leading dimension of
        out in doubles; r16: the round16 bits (_gram_bits)."""
        lib = _lib.load()
        n, nb, step = xi.shape[0], x_bdy.shape[0], int(self.cross_rows_per_call)
        for lo in range(0, n, step):
            _lib.check(lib.scasml_gp_cross_rows(self.d, self.a, _lib.ptr(x_dom), x_dom.shape[0], _lib.ptr(x_bdy) if nb else None, nb, self._idx_ptr, r16,
                                                0 if self.compat == "reference" else 1, op, _lib.ptr(xi[lo:]), min(step, n - lo), self.d + 1,
                                                _lib.ptr(out[lo:]), ld, _lib.stream_ptr()), "gp_cross_rows")

    def _solved_rows(self, L, xi, r16, buf, var):
        """buf[:len(xi)] <- (L^-1 K(phi, x_i))^T: op-0 feature rows solved in place by scasml_gp_variance (its variances, a by-product, go to var).
        buf, (rows x Mp), was ZEROED when it was allocated: the feature rows fill columns 0 .. M, and columns M .. Mp stay zero through every
        solve, because L is the identity there."""
        n, Mp = xi.shape[0], L.shape[0]
        self._cross_rows(self._xd, self._xb, 0, xi, buf, Mp, r16)
        _lib.check(_lib.load().scasml_gp_variance(_lib.ptr(L), Mp, _lib.ptr(buf), Mp, n, 1.0, _lib.ptr(var), _lib.stream_ptr()), "gp_variance")
        return buf[:n]

    def _prior_block(self, xi, yi, f16_ops):
        """kappa(x_i, y_j), (n, m) float64 on the device.  Documented operators: exp(-a |x - y|^2 / 2) in float64, the squared distance added
        coordinate by coordinate.  As coded: the library's own op-0 entry for the pair, by kappa_kernel's route -- scasml_gp_cross_rows with the y
        block as a domain set, whose first m columns are kappa -- walked in column blocks that keep its (n x 4 m) rows under
        variance_buffer_bytes.  f16_ops (f16_graph, x AND y handed in as float16 arrays) selects the reference's float16 op sequence; it is decided
        by the callers' dtypes, never by the values of a block, so every entry is a function of its own pair, whatever the block."""
        torch = _lib.require_gpu()
        n, m = xi.shape[0], yi.shape[0]
        if self.compat is None:
            x64, y64 = xi.to(torch.float64), yi.to(torch.float64)
            dist = torch.zeros((n, m), dtype=torch.float64, device="cuda")
            for k in range(self.d + 1):
                diff = x64[:, k:k + 1] - y64[None, :, k]
                dist.addcmul_(diff, diff)
            return dist.mul_(-0.5 * self.a).exp_()
        out = torch.empty((n, m), dtype=torch.float64, device="cuda")
        r16 = _lib.ROUND16_ENTRIES | (_lib.ROUND16_F16_OPS | self._f16_extra if f16_ops else 0)
        step = int(max(1, min(m, self.variance_buffer_bytes // (32 * n))))
        rows = torch.empty((n, 4 * step), dtype=torch.float64, device="cuda")
        for lo in range(0, m, step):
            w = min(step, m - lo)
            self._cross_rows(yi[lo:lo + w], yi[:0], 0, xi, rows, 4 * step, r16)
            out[:, lo:lo + w] = rows[:, :w]
        return out

    def predict_covariance(self, x_t_infer, y_t_infer=None):
        '''(n, m) float64 posterior covariance  cov(x_i, y_j) = kappa(x_i, y_j) - (L^-1 K(phi, x_i))^T (L^-1 K(phi, y_j));  y = None means y = x
        (NumPy in, NumPy out; CUDA tensor in, CUDA tensor out; the raw value, not clamped).

        compat=None: the posterior covariance of u under the prior kappa given noisy observations of the collocation functionals.
        compat="reference": the as-coded ANALOGUE, with the caveat of predict_variance -- the same formula on the matrices the reference's code
        builds, which are not the Gram matrix and cross-covariances of one kernel: no positive semidefiniteness is guaranteed (sample_posterior's
        jitter covers it).  The prior entry is then the library's own as-coded kappa for the pair (kappa_kernel's route); under f16_graph it follows the
        float16 op sequence when x and y are both handed in as float16 arrays -- decided by the dtypes, not by the values.

        Composed from what predict_variance uses: scasml_gp_cross_rows (op 0) into padded row buffers, scasml_gp_variance solves each in place
        (rows <- rows L^-T), the prior block goes into C and scasml_gemm_nt_sub subtracts Vx Vy^T on the FP64 matrix cores (K = Mp, a fixed sum
        order).  Every entry is a function of its own pair of points, bit for bit: a sub-selection, a permutation or another chunking returns the
        same bits.  With y = None the solved rows are computed once, one triangle is computed and mirrored: C == C.T exactly, and the same bits as
        predict_covariance(x, x).  diag(C) agrees with predict_variance to ROUNDING only -- that kernel sums the squares column by column in one
        register, this one in the MFMA's 4-wide order.  n and m are walked in chunks so that both row buffers together stay under
        ``variance_buffer_bytes``.'''
        torch = _lib.require_gpu()
        lib = _lib.load()
        L = self._variance_factor()
        xi, was_numpy, f16x = self._rows_device(x_t_infer)
        symmetric = y_t_infer is None
        yi, f16y = (xi, f16x) if symmetric else self._rows_device(y_t_infer)[::2]
        n, m, Mp = xi.shape[0], yi.shape[0], L.shape[0]
        Cm = torch.empty((n, m), dtype=torch.float64, device="cuda")
        if n == 0 or m == 0:
            return Cm.cpu().numpy() if was_numpy else Cm
        rows_cap = int(max(2, self.variance_buffer_bytes // (8 * Mp)))
        s = _lib.stream_ptr()
        f16_ops = self.f16_graph and f16x and f16y
        r16x = self._gram_bits(self._xd, self._xb, f16x)
        r16y = r16x if symmetric else self._gram_bits(self._xd, self._xb, f16y)

        def subtract(block, Vx, Vy, lower_only):
            # lower_only (a diagonal block of the symmetric case): the 64 x 64 tiles above the 256-row block diagonal are skipped, then mirrored over
            _lib.check(lib.scasml_gemm_nt_sub(_lib.ptr(block), block.stride(0), block.shape[0], block.shape[1], _lib.ptr(Vx), Mp, _lib.ptr(Vy), Mp, Mp,
                                              0, 1 if lower_only else 0, 0, s), "gemm_nt_sub")

        if symmetric and n <= rows_cap:
            Vx = self._solved_rows(L, xi, r16x, torch.zeros((n, Mp), dtype=torch.float64, device="cuda"), torch.empty(n, dtype=torch.float64, device="cuda"))
            Cm.copy_(self._prior_block(xi, xi, f16_ops))
            subtract(Cm, Vx, Vx, True)
        else:
            cx = int(min(n, rows_cap // 2))
            cy = int(min(m, rows_cap // 2))
            bx = torch.zeros((cx, Mp), dtype=torch.float64, device="cuda")           # zeroed here, once (_solved_rows)
            by = torch.zeros((cy, Mp), dtype=torch.float64, device="cuda")
            var = torch.empty(max(cx, cy), dtype=torch.float64, device="cuda")
            for i0 in range(0, n, cx):
                Vx = self._solved_rows(L, xi[i0:i0 + cx], r16x, bx, var)
                for j0 in range(0, m, cy):
                    if symmetric and j0 > i0:                          # cx == cy: the blocks above the diagonal are mirrored
                        break
                    diag = symmetric and j0 == i0
                    Vy = Vx if diag else self._solved_rows(L, yi[j0:j0 + cy], r16y, by, var)
                    block = Cm[i0:i0 + cx, j0:j0 + cy]
                    block.copy_(self._prior_block(xi[i0:i0 + cx], yi[j0:j0 + cy], f16_ops))
                    subtract(block, Vx, Vy, diag)
        if symmetric:
            Cm = torch.tril(Cm) + torch.tril(Cm, -1).t()
        return Cm.cpu().numpy() if was_numpy else Cm

    def sample_posterior(self, x_t_infer, n_samples, seed=0, jitter=None, sample0=0):
        '''(n_samples, n) float64 draws from N(mean(x), cov(x, x) + jitter I) (NumPy in, NumPy out; CUDA tensor in, CUDA tensor out).

        mean = predict(x) widened to float64 -- the surrogate the solvers use, float16 output values as coded included; cov = predict_covariance(x).
        The covariance is copied into an identity-padded buffer and factored by scasml_cholesky with nugget = jitter (default: self.nugget, the
        observation noise the model already assumes, which also keeps the as-coded analogue factorable); a non-positive pivot raises ValueError.
        scasml_gp_sample then forms mean + Lc z on the FP64 matrix cores with Philox normals drawn inside the kernel: draw s is a function of
        (x, seed, sample0 + s) alone, bit for bit, so the chunks n_samples is walked in (host output: the device holds one chunk at a time) cannot change it and
        ``sample0`` continues a stream of draws.  n is bounded by the n x n factor: 8 np^2 bytes (np = n rounded up to 32) must fit ``variance_buffer_bytes``.'''
        torch = _lib.require_gpu()
        lib = _lib.load()
        n_samples, sample0 = int(n_samples), int(sample0)
        if n_samples < 0 or sample0 < 0:
            raise ValueError("n_samples and sample0 must not be negative")
        jitter = float(self.nugget if jitter is None else jitter)
        was_numpy = not isinstance(x_t_infer, torch.Tensor)
        # the caller's rows in their own dtype, on the device once (float16 rows stay float16 rows for predict and the as-coded entries)
        xdev = torch.from_numpy(np.ascontiguousarray(np.asarray(x_t_infer))).cuda() if was_numpy else x_t_infer
        self._check_rows(xdev)
        n = xdev.shape[0]
        npad = _round_up(max(n, 1), 32)
        if 8 * npad * npad > self.variance_buffer_bytes:
            raise ValueError("sample_posterior factors an n x n covariance: n = %d needs %d bytes, variance_buffer_bytes = %d allows n <= %d" % (
                n, 8 * npad * npad, self.variance_buffer_bytes, int(np.sqrt(self.variance_buffer_bytes // 8)) // 32 * 32))
        if n == 0 or n_samples == 0:
            return np.empty((n_samples, n)) if was_numpy else torch.empty((n_samples, n), dtype=torch.float64, device="cuda")
        mean = self.predict(xdev)[:, 0].to(torch.float64).contiguous()
        Lc, info = self._factor_padded(self.predict_covariance(xdev), jitter, "cholesky(cov)")
        if info != 0:
            raise ValueError("cov(x, x) + jitter I is not positive definite at jitter = %g (pivot %d of %d): pass a larger jitter" % (jitter, info, n))
        s = _lib.stream_ptr()
        seed = int(seed) & 0xFFFFFFFFFFFFFFFF
        if not was_numpy:                                              # the caller's tensor is the whole output anyway: one launch
            out = torch.empty((n_samples, n), dtype=torch.float64, device="cuda")
            _lib.check(lib.scasml_gp_sample(_lib.ptr(Lc), npad, n, _lib.ptr(mean), seed, sample0, n_samples, _lib.ptr(out), n, s), "gp_sample")
            return out
        # host output: the device holds one chunk of draws at a time, under variance_buffer_bytes
        chunk = int(min(n_samples, max(64, self.variance_buffer_bytes // (8 * n) // 64 * 64)))
        out, dev = np.empty((n_samples, n)), torch.empty((chunk, n), dtype=torch.float64, device="cuda")
        for lo in range(0, n_samples, chunk):
            c = min(chunk, n_samples - lo)
            _lib.check(lib.scasml_gp_sample(_lib.ptr(Lc), npad, n, _lib.ptr(mean), seed, sample0 + lo, c, _lib.ptr(dev), n, s), "gp_sample")
            out[lo:lo + c] = dev[:c].cpu().numpy()
        return out

    # pathwise posterior draws (no counterpart in models/GP.py): functions, not vectors -- a random-Fourier-feature prior draw plus the data term
    def _rff_functionals(self, xi, n_features, seed, sample0, S):
        """(S, n, 4) float64 device tensor: u, Lap, dt, div of the prior draws sample0 .. sample0 + S at the float32 device rows xi."""
        torch = _lib.require_gpu()
        out = torch.empty((S, xi.shape[0], 4), dtype=torch.float64, device="cuda")
        if out.numel():
            _lib.check(_lib.load().scasml_gp_rff_functionals(self.d, self.a, _lib.ptr(xi), xi.shape[0], xi.stride(0), int(n_features),
                                                             int(seed) & 0xFFFFFFFFFFFFFFFF, int(sample0), S, _lib.ptr(out), _lib.stream_ptr()),
                       "gp_rff_functionals")
        return out

    def _rff_gradient(self, xi, n_features, seed, sample0, S):
        """(S, n, d+1) float64 device tensor: the gradient of the prior draws sample0 .. sample0 + S at the float32 device rows xi."""
        torch = _lib.require_gpu()
        out = torch.empty((S, xi.shape[0], self.d + 1), dtype=torch.float64, device="cuda")
        if out.numel():
            _lib.check(_lib.load().scasml_gp_rff_gradient(self.d, self.a, _lib.ptr(xi), xi.shape[0], xi.stride(0), int(n_features),
                                                          int(seed) & 0xFFFFFFFFFFFFFFFF, int(sample0), S, _lib.ptr(out), self.d + 1, _lib.stream_ptr()),
                       "gp_rff_gradient")
        return out

    def _data_gradient(self, xi, neg, prior=None):
        """(S, n, d+1) float64 on the device: the gradient in x of k(x, phi)^T v_s at the float32 device rows xi, time derivative last, for the S
        vectors v_s = -neg[s, :M] (neg: (S, Mp) float64, the padding zero: what scasml_gemm_nt_sub takes); prior(xc) -> (S, c, d+1), if given, is
        added chunk by chunk.  compat=None only.

        With c0, cL, ct, cS the u, Lap, dt, div entries of v_s per collocation point y_j (boundary points: c0 only), K0 the op-0 cross rows and
        r = x_i - y_j (gp_gradient_kernel's identity, in float64 and without the n x M x (d+1) rows of op 4):
            kE_ij = K0[i,u_j] c0_j + K0[i,Lap_j] cL_j + K0[i,dt_j] ct_j + K0[i,div_j] cS_j        alpha_ij = a (2a K0[i,u_j] cL_j - kE_ij)
            d_k = x_ik sum_j alpha_ij - sum_j alpha_ij y_jk + a sum_j K0[i,u_j] cS_j   (k < d)      d_t = (op-2 row) . v_s
        alpha is elementwise torch (_gradient_alpha_pass); every sum over j is a scasml_gemm_nt_sub (alpha against the collocation coordinates and a
        row of ones, K0 against a cS_j, the op-2 rows against v), whose row i depends on row i of its operands alone -- so a point's values are the
        same bits however the points are split, permuted or chunked.  x is walked in chunks that keep a (points x Mp) row buffer under
        variance_buffer_bytes."""
        torch = _lib.require_gpu()
        d, a, N, Nb = self.d, self.a, self.N_domain, self.N_boundary
        S, n, Mp = neg.shape[0], xi.shape[0], neg.shape[1]
        out = torch.empty((S, n, d + 1), dtype=torch.float64, device="cuda")
        if S == 0 or n == 0:
            return out
        f64 = dict(dtype=torch.float64, device="cuda")
        Np = _round_up(N + Nb, 32)
        yext = torch.zeros((d + 1, Np), **f64)                                   # rows 0 .. d: the collocation coordinates; row d: ones
        yext[:d, :N] = self._xd[:, :d].t()
        yext[:d, N:N + Nb] = self._xb[:, :d].t()
        yext[d, :N + Nb] = 1.0
        neg_div = torch.zeros((S, Mp), **f64)                                    # C -= K0 neg_div^T adds a sum_j K0[i,u_j] cS_j
        neg_div[:, :N] = a * neg[:, 3 * N + Nb:4 * N + Nb]
        chunk = int(max(1, min(self.variance_buffer_bytes // (8 * Mp), self.cross_rows_per_call, n)))
        rows = torch.zeros((chunk, Mp), **f64)                                   # columns M .. Mp stay zero: the cross rows fill 0 .. M
        x64 = xi[:, :d].to(torch.float64)
        for lo in range(0, n, chunk):
            xc = xi[lo:lo + chunk]
            c = xc.shape[0]
            tail = torch.zeros((c, 2, S), **f64)                                 # [:, 0, s] = d_t,  [:, 1, s] = a sum_j K0[i,u_j] cS_j
            self._cross_rows(self._xd, self._xb, 2, xc, rows, Mp, 0)
            self._gemm_nt_sub(tail[:, 0, :], rows, Mp, neg, Mp)
            self._cross_rows(self._xd, self._xb, 0, xc, rows, Mp, 0)
            self._gemm_nt_sub(tail[:, 1, :], rows, Mp, neg_div, Mp)
            self._gradient_alpha_pass(rows[:c], x64[lo:lo + c], neg, yext, tail, out[:, lo:lo + c])
            if prior is not None:
                out[:, lo:lo + c] += prior(xc)
        return out

    @staticmethod
    def _gemm_nt_sub(Cm, A, lda, B, K):
        """Cm (its own shape and row stride) -= A (lda) B^T over K columns: the one call of scasml_gemm_nt_sub of the gradient routines."""
        _lib.check(_lib.load().scasml_gemm_nt_sub(_lib.ptr(Cm), Cm.stride(0), Cm.shape[0], Cm.shape[1], _lib.ptr(A), lda, _lib.ptr(B), B.stride(0), K,
                                                  0, 0, 0, _lib.stream_ptr()), "gemm_nt_sub")

    def _gradient_alpha_pass(self, K0, x64, neg, yext, tail, out):
        """out (S, c, d+1) <- the data-term gradient of one chunk from its op-0 rows K0 (c, Mp), its spatial coordinates x64 (c, d) and tail (c, 2, S)
        (_data_gradient).  The draws go in groups that keep alpha and its two temporaries, (group x c x N) doubles each, under variance_buffer_bytes:
        alpha is elementwise torch over the whole group, and ONE scasml_gemm_nt_sub of its (group c) rows against [Y, 1] sums over j."""
        torch = _lib.require_gpu()
        d, a, N, Nb = self.d, self.a, self.N_domain, self.N_boundary
        S, c, Np = neg.shape[0], K0.shape[0], yext.shape[1]
        ku, kb = K0[None, :, :N], K0[None, :, N:N + Nb]
        kL, kt, kS = (K0[None, :, k * N + Nb:(k + 1) * N + Nb] for k in (1, 2, 3))
        group = int(max(1, min(S, self.variance_buffer_bytes // (24 * Np * c))))
        for j0 in range(0, S, group):
            v = -neg[j0:j0 + group, None, :]                                     # (g, 1, Mp): the group's vectors
            g = v.shape[0]
            c0, c0b = v[:, :, :N], v[:, :, N:N + Nb]
            cL, ct, cS = (v[:, :, k * N + Nb:(k + 1) * N + Nb] for k in (1, 2, 3))
            alpha = torch.zeros((g, c, Np), dtype=torch.float64, device="cuda")  # columns N + Nb .. Np stay zero
            kE = ku * c0
            kE.addcmul_(kL, cL).addcmul_(kt, ct).addcmul_(kS, cS)
            alpha[:, :, :N] = (ku * (2.0 * a * cL)).sub_(kE).mul_(a)
            alpha[:, :, N:N + Nb] = kb * (-a * c0b)
            acc = torch.zeros((g, c, d + 1), dtype=torch.float64, device="cuda")  # <- -alpha [Y, 1]: columns k < d, then -sum_j alpha_ij
            self._gemm_nt_sub(acc.view(g * c, d + 1), alpha, Np, yext, Np)
            t = tail[:, :, j0:j0 + g].permute(2, 0, 1)                           # (g, c, 2)
            out[j0:j0 + g, :, :d] = acc[:, :, :d] - x64[None] * acc[:, :, d:] + t[:, :, 1:]
            out[j0:j0 + g, :, d] = t[:, :, 0]

    def posterior_mean_gradient(self, x_t_infer):
        '''(n, d+1) float64 gradient of the posterior mean k(x, phi)^T right_vector, time derivative last (NumPy in, NumPy out; CUDA tensor in,
        CUDA tensor out): the float64 statement of compute_gradient, which is the float32 kernel the solvers use and does not change.  The data
        term of GPFunctionDraws.gradient applied to right_vector (_data_gradient); every point's values are a function of that point alone, bit for
        bit.  compat=None only.'''
        torch = _lib.require_gpu()
        if self.compat == "reference":
            raise ValueError("posterior_mean_gradient needs compat=None: the as-coded matrix is not the Gram of one kernel and has no spectral density")
        self._require_trained()
        xi, was_numpy, _ = self._rows_device(x_t_infer)
        neg = torch.zeros((1, _round_up(self.phi_dim, 32)), dtype=torch.float64, device="cuda")
        neg[0, :self.phi_dim] = -torch.from_numpy(np.ascontiguousarray(self.right_vector, dtype=np.float64).reshape(-1)).cuda()
        out = self._data_gradient(xi, neg)[0]
        return out.cpu().numpy() if was_numpy else out

    def sample_functions(self, n_samples, seed=0, n_features=2048, sample0=0, z=None):
        '''n_samples posterior draws as functions (GPFunctionDraws: .right_vectors, .predict(x), .functionals(x)), by pathwise conditioning
        (Matheron's rule; Wilson et al., ICML 2020):
            post_s(x) = f_s(x) + k(x, phi)^T K_p^-1 (z - Phi[f_s] - sqrt(nugget) eps_s)
        f_s is a prior draw from n_features random Fourier features of its own (scasml_gp_rff_functionals, csrc/gp_rff.hip), Phi[f_s] its collocation
        functionals in the Gram's order [u(dom), u(bdy), Lap(dom), dt(dom), div(dom)], eps_s ~ N(0, I) (scasml_gp_rff_noise) and z the feature
        values (default: those of log_marginal_likelihood -- b(sol) of the fit, else K_p right_vector).  The S right-hand sides are solved with the cached factor
        (two scasml_trsm_lower calls, nrhs = S).  Mean and covariance of the draws are exactly k K_p^-1 z and predict_covariance for every
        n_features; only the Gaussianity of the joint is asymptotic in it.  The mean part is the float64 statement k(x)^T right_vector, not the bf16
        evaluation of GP.predict.  Unlike sample_posterior nothing n x n is factored: the cost is linear in the points, a draw can be evaluated
        anywhere, again, and differentiated (Lap, dt, div, and so its PDE residual).  Draw s is a function of (model, seed, sample0 + s, n_features)
        alone.  compat=None only.'''
        torch = _lib.require_gpu()
        lib = _lib.load()
        if self.compat == "reference":
            raise ValueError("pathwise draws need compat=None: the as-coded matrix is not the Gram of one kernel and has no spectral density")
        if getattr(self, "_xd", None) is None:
            raise _lib.ScasmlError("no collocation points yet: call GPsolver / kernel_phi_phi / load_right_vector first")
        S, F, sample0 = int(n_samples), int(n_features), int(sample0)
        if S < 0 or sample0 < 0:
            raise ValueError("n_samples and sample0 must not be negative")
        if F < 1 or F >= 1 << 31:
            raise ValueError("n_features must lie in 1 .. 2^31 - 1, got %d" % F)
        if sample0 + S > 1 << 32:
            raise ValueError("draw indices %d .. %d reach 2^32 (the Philox root word is 32 bits)" % (sample0, sample0 + S - 1))
        zt = self._evidence_z(z)
        L = self._variance_factor()
        N, Nb, M, Mp = self.N_domain, self.N_boundary, self.phi_dim, L.shape[0]
        s = _lib.stream_ptr()
        seed = int(seed) & 0xFFFFFFFFFFFFFFFF
        rhs = torch.zeros((S, Mp), dtype=torch.float64, device="cuda")
        if S:
            _lib.check(lib.scasml_gp_rff_noise(M, seed, sample0, S, _lib.ptr(rhs), Mp, s), "gp_rff_noise")
            rhs[:, :M].mul_(-float(np.sqrt(self.nugget))).add_(zt)
            fd = self._rff_functionals(self._xd, F, seed, sample0, S)
            rhs[:, :N] -= fd[:, :, 0]
            if Nb:
                rhs[:, N:N + Nb] -= self._rff_functionals(self._xb, F, seed, sample0, S)[:, :, 0]
            for k in (1, 2, 3):
                rhs[:, k * N + Nb:(k + 1) * N + Nb] -= fd[:, :, k]
            B = rhs.t().contiguous()                                   # (Mp, S): the right-hand sides as columns
            for trans in (0, 1):
                _lib.check(lib.scasml_trsm_lower(_lib.ptr(L), Mp, _lib.ptr(B), S, trans, s), "trsm_lower")
            rhs = B.t()
        return GPFunctionDraws(self, rhs[:, :M].contiguous(), F, seed, sample0)

    def compute_gradient(self, x_t_infer, sol_infer=None):
        '''(n, d+1) gradient of the posterior mean, time derivative last (models/GP.py:673-687).'''
        torch = _lib.require_gpu()
        lib = _lib.load()
        pts, was_numpy, _, _ = self._points_device(x_t_infer)
        grad = torch.empty((pts.shape[0], self.d + 1), dtype=torch.float32, device="cuda")
        if self.compat is None:
            model = self._device_model()
            _lib.check(lib.scasml_gp_gradient(C.byref(model), _lib.ptr(pts), pts.shape[0], _lib.ptr(grad), _lib.stream_ptr()), "gp_gradient")
        else:      # autodiff of the as-coded u_hat (through the float16 casts); any nonzero round16 casts the result to float16 (:687)
            _lib.check(lib.scasml_gp_gradient_compat(self.d, self.a, *self._f64_model(), _lib.ROUND16_ENTRIES, _lib.ptr(pts), pts.shape[0],
                                                     pts.shape[1], _lib.ptr(grad), _lib.stream_ptr()), "gp_gradient_compat")
        return grad.cpu().numpy() if was_numpy else grad

    def compute_PDE_loss(self, x_t_infer):
        raise NotImplementedError

    # ------------------------------------------------------------------ the cross-kernel builders of the reference's class surface
    # (models/GP.py:41-179, 271-411, 630-651).  The hot path never materialises these matrices -- predict / compute_PDE_loss contract them on the
    # fly -- but callers of the reference's methods find them here, as host views over scasml_gp_cross_rows.  With compat="reference" the entries
    # are float16 VALUES (returned as float16, like the reference's .astype(jnp.float16)); with compat=None float64, not rounded.
    _OPS = {"I": 0, "lap": 1, "dt": 2, "div": 3}

    def _cross(self, op, x_t_infer, x_t_domain, x_t_boundary):
        """(N_inf, M) rows of operator `op` (or, op = 4, the (N_inf, M, d+1) gradient of the op-0 rows) against the given collocation sets."""
        torch = _lib.require_gpu()
        xi, was_numpy, f16_rows = self._rows_device(x_t_infer, flat=True)
        xd = self._rows_device(x_t_domain, flat=True)[0]
        xb = self._rows_device(x_t_boundary, flat=True)[0] if x_t_boundary is not None and len(x_t_boundary) else xd[:0]
        if xd.shape[0] < 1:
            raise ValueError("the cross-kernel builders need at least one domain point")
        ni, M = xi.shape[0], 4 * xd.shape[0] + xb.shape[0]
        out = torch.empty((ni, M, self.d + 1) if op == 4 else (ni, M), dtype=torch.float64, device="cuda")
        self._cross_rows(xd, xb, op, xi, out, M, self._gram_bits(xd, xb, f16_rows))
        if self.compat == "reference":
            out = out.to(torch.float16)                               # exact: the entries are float16 values
        return out.cpu().numpy() if was_numpy else out

    def kernel_x_t_phi(self, x_t_infer, x_t_domain, x_t_boundary):
        '''K(x_t, phi): (N_infer, 4 N_domain + N_boundary), columns [kappa(dom), kappa(bdy), lap_y kappa, dt_y kappa, div_y kappa] (models/GP.py:271-294).'''
        return self._cross(0, x_t_infer, x_t_domain, x_t_boundary)

    def dx_t_kernel_x_t_phi(self, x_t_infer, x_t_domain, x_t_boundary):
        '''Gradient of K(x_t, phi) in x_t: (N_infer, 4 N_domain + N_boundary, n_input), time derivative last (models/GP.py:296-324).'''
        return self._cross(4, x_t_infer, x_t_domain, x_t_boundary)

    def laplacian_x_t_kernel_x_t_phi(self, x_t_infer, x_t_domain, x_t_boundary):
        '''The Laplacian feature rows (as coded: the 5-index Hutchinson sum on the shifted argument) (models/GP.py:326-354).'''
        return self._cross(1, x_t_infer, x_t_domain, x_t_boundary)

    def dt_x_t_kernel_x_t_phi(self, x_t_infer, x_t_domain, x_t_boundary):
        '''The time-derivative feature rows (models/GP.py:356-383).'''
        return self._cross(2, x_t_infer, x_t_domain, x_t_boundary)

    def div_x_t_kernel_x_t_phi(self, x_t_infer, x_t_domain, x_t_boundary):
        '''The divergence feature rows (models/GP.py:385-411).'''
        return self._cross(3, x_t_infer, x_t_domain, x_t_boundary)

    def kernel_x_t_phi_single(self, x_t):
        '''K(x_t, phi) for one point against the fitted collocation sets: (4 N_domain + N_boundary,) (models/GP.py:630-651).'''
        if getattr(self, "x_t_domain", None) is None:
            raise _lib.ScasmlError("no collocation points yet: call GPsolver / kernel_phi_phi / load_right_vector first")
        torch = _lib.require_gpu()
        row = x_t.reshape(1, -1) if isinstance(x_t, torch.Tensor) else np.asarray(x_t).reshape(1, -1)
        return self._cross(0, row, self.x_t_domain, self.x_t_boundary)[0]

    def _pair(self, opx, opy, x_t, y_t):
        """(L^opx_x L^opy_y kappa)(x_t, y_t) for single vectors: y_t plays a one-point domain set, whose row holds all four y-operators."""
        torch = _lib.require_gpu()
        x = x_t.reshape(1, -1) if isinstance(x_t, torch.Tensor) else np.asarray(x_t).reshape(1, -1)
        y = y_t.reshape(1, -1) if isinstance(y_t, torch.Tensor) else np.asarray(y_t).reshape(1, -1)
        if opx == "grad":
            g = self._cross(4, x, y, None)[0, 0]
            return g
        return self._cross(self._OPS[opx], x, y, None)[0, self._OPS[opy]]

    def kappa(self, x_t, y_t):
        '''K(x_t, y_t) for single vectors (models/GP.py:41-43).'''
        return self._pair("I", "I", x_t, y_t)

    def kappa_kernel(self, x_t, y_t):
        '''(N_x, N_y) kernel matrix (models/GP.py:45-53).'''
        return self._cross(0, x_t, y_t, None)[:, :len(y_t)]

    def dx_t_kappa(self, x_t, y_t):
        '''Gradient of kappa in x_t, (n_input,) (models/GP.py:55-57).'''
        return self._pair("grad", None, x_t, y_t)

    def dy_t_kappa(self, x_t, y_t):
        '''Gradient of kappa in y_t = -gradient in x_t (models/GP.py:65-67).'''
        return -self._pair("grad", None, x_t, y_t)


def _pair_method(name, opx, opy, cite):
    def method(self, x_t, y_t):
        return self._pair(opx, opy, x_t, y_t)
    method.__name__ = name
    method.__doc__ = "(L^%s_x L^%s_y kappa)(x_t, y_t) for single vectors (models/GP.py:%s)." % (opx, opy, cite)
    return method


# the derivative kernels of the reference's class surface, by (operator in x, operator in y): one host view each
for _name, _ox, _oy, _cite in (
        ("dt_x_t_kappa", "dt", "I", "59-63"), ("dt_y_t_kappa", "I", "dt", "69-73"), ("div_x_kappa", "div", "I", "75-79"), ("div_y_kappa", "I", "div", "81-85"),
        ("laplacian_x_t_kappa", "lap", "I", "87-95"), ("laplacian_y_t_kappa", "I", "lap", "97-105"), ("dt_x_t_dt_y_t_kappa", "dt", "dt", "107-111"),
        ("dt_x_t_div_y_kappa", "dt", "div", "113-117"), ("dt_x_t_laplacian_y_t_kappa", "dt", "lap", "119-127"), ("div_x_dt_y_t_kappa", "div", "dt", "129-133"),
        ("div_x_div_y_kappa", "div", "div", "135-139"), ("div_x_laplacian_y_t_kappa", "div", "lap", "141-149"),
        ("laplacian_x_t_dt_y_t_kappa", "lap", "dt", "151-159"), ("laplacian_x_t_div_y_kappa", "lap", "div", "161-169"),
        ("laplacian_x_t_laplacian_y_t_kappa", "lap", "lap", "171-179")):
    setattr(GP, _name, _pair_method(_name, _ox, _oy, _cite))
del _name, _ox, _oy, _cite


class GP_Semilinear(GP):
    '''The surrogate for any registered equation of the family u_t + mu div u + sigma^2/2 Lap u + f(u, sum z) = 0
    (csrc/equations.hpp): the reference has one concrete subclass per PDE (models/GP.py:693-769 for
    Grad_Dependent_Nonlinear); here the equation's eq_id selects F and f inside the kernels.'''

    def rhs_f(self, x_t):
        return np.zeros((np.asarray(x_t).shape[0],), dtype=np.float64)     # :700-702

    def time_der_rep(self, sol, rhs_f):
        '''F(z) = -mu z5 - (sigma^2/2) z3 - f(z1, sigma z5) + rhs_f; for Grad_Dependent_Nonlinear
        -sigma^2 z1 z5 + (1/d + sigma^2/2) z5 - (sigma^2/2) z3 + rhs_f  (:705-719)'''
        N = self.N_domain
        sol = np.asarray(sol, dtype=np.float64)
        return self.equation.F_parts(sol[:N], sol[N:2 * N], sol[2 * N:])[0] + rhs_f

    def DF_domain_without_time(self, sol):
        '''Jacobian of F in the unknowns (z1, z3, z5): (N, 3N) = [diag dF/dz1 | diag dF/dz3 | diag dF/dz5], float16 as the reference returns it
        (models/GP.py:722-743).  Host NumPy; the device Newton uses the same derivatives through eq_F (csrc/equations.hpp).'''
        N = self.N_domain
        sol = np.asarray(sol, dtype=np.float64).reshape(-1)
        d1, d3, d5 = self.equation.F_parts(sol[:N], sol[N:2 * N], sol[2 * N:])[1]
        return np.hstack([np.diag(np.broadcast_to(v, (N,))) for v in (d1, d3, d5)]).astype(np.float16)

    def compute_PDE_loss(self, x_t_infer):
        '''dt u + mu div u + sigma^2/2 Lap u + f(u, sigma div u); for Grad_Dependent_Nonlinear
        dt u + (sigma^2 u - 1/d - sigma^2/2) div u + sigma^2/2 Lap u  (models/GP.py:746-769)'''
        pts, was_numpy, hb, f16 = self._points_device(x_t_infer)
        out = self._eval_device(pts, hb, f16)[:, 2:3]
        return out.cpu().numpy() if was_numpy else out


class GP_Grad_Dependent_Nonlinear(GP_Semilinear):
    '''Gaussian Kernel Solver for the Grad_Dependent_Nonlinear (models/GP.py:693-769)'''


class GP_Cubic_Reaction_Diffusion(GP_Semilinear):
    '''The surrogate of equations.Cubic_Reaction_Diffusion (eq_id 1).'''
