"""Block-row distributed Gram / Cholesky / solves / Newton-CG (scasml_gp_amd/dist_gp.py, csrc/dist_linalg.hip) against the
single-GPU path: world = 1 in process, and world = 2 / 3 as processes that share the test box's one GPU and meet over gloo
(the RCCL run needs the 8-GPU node the driver owns)."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def _problem(d, nd, nb, seed=1234):
    from scasml_gp_amd.equations.equations import Grad_Dependent_Nonlinear
    eq = Grad_Dependent_Nonlinear(d + 1)
    state = np.random.get_state()
    np.random.seed(seed)
    dom, bdy = eq.generate_data(nd, nb)
    np.random.set_state(state)
    return eq, dom, bdy


def _single_gpu_factor(eq, dom, bdy):
    from scasml_gp_amd.models.GP import GP_Grad_Dependent_Nonlinear
    gp = GP_Grad_Dependent_Nonlinear(eq, compat=None)
    gp.kernel_phi_phi(dom, bdy)
    return gp, gp.cholesky_phi_phi_perturb


def _check_against_single_gpu(ch, L, tol):
    """max |R - L| over this rank's block rows, relative to max |L|."""
    import torch
    from scasml_gp_amd.dist_gp import BLK
    worst = 0.0
    for slot, i in enumerate(ch.mine):
        r0, r1 = i * BLK, min((i + 1) * BLK, ch.M)
        if r1 <= r0:
            continue
        mine = torch.tril(ch.R[slot * BLK:slot * BLK + (r1 - r0), :ch.M], diagonal=r0)
        worst = max(worst, float((mine - L[r0:r1]).abs().max()))
    scale = float(L.abs().max())
    assert worst <= tol * scale, (worst, scale)
    return worst / scale


def test_world1_factor_and_solve_match_the_single_gpu_path():
    import torch
    from scasml_gp_amd import _lib
    from scasml_gp_amd.dist_gp import DistCholesky
    eq, dom, bdy = _problem(20, 500, 100)
    gp, L = _single_gpu_factor(eq, dom, bdy)
    ch = DistCholesky(20, 1.0 / float(gp.sigma) ** 2, dom, bdy, gp.nugget).build().factor()
    assert ch.M == 2100 and ch.nblk == 9 and len(ch.mine) == 9
    _check_against_single_gpu(ch, L, 1e-12)
    # the look-ahead (next block column's chain on a second stream) only reorders independent work: bit-identical factor
    plain = DistCholesky(20, 1.0 / float(gp.sigma) ** 2, dom, bdy, gp.nugget).build().factor(lookahead=False)
    torch.cuda.synchronize()
    assert torch.equal(plain.R, ch.R) and all(torch.equal(a, b) for a, b in zip(plain.diag, ch.diag))
    # block columns one at a time (round 5's sequence) and in pairs (one K = 512 trailing update per pair, the default): the same factor to rounding,
    # (9 block rows: four pairs and a last odd column)
    single = DistCholesky(20, 1.0 / float(gp.sigma) ** 2, dom, bdy, gp.nugget).build().factor(pair=False)
    torch.cuda.synchronize()
    assert float((single.R - ch.R).abs().max()) <= 1e-13 * float(ch.R.abs().max())
    del single, plain
    Lg = ch.gather_factor()
    assert float((Lg - L).abs().max()) <= 1e-12 * float(L.abs().max())
    b = torch.from_numpy(np.random.default_rng(0).standard_normal(ch.M)).cuda()
    x = ch.solve(b)
    Kp = L @ L.T
    assert float((Kp @ x - b).abs().max()) <= 1e-9 * float(b.abs().max())
    assert float((ch.matvec(b) - Kp @ b).abs().max()) <= 1e-11 * float((Kp @ b).abs().max())


@pytest.mark.parametrize("row0,nrows,ncols", [(0, 630, 630), (100, 300, 400), (170, 20, 190), (329, 257, 586), (480, 150, 37), (629, 1, 630)])
def test_gram_rows_tile_kernel_equals_the_rows_of_the_full_gram(row0, nrows, ncols):
    """scasml_gp_gram_rows (FP64-MFMA pair tiles, one launch per operator segment of the row range) against the same rows of
    scasml_gp_gram, for ranges that start and end inside, and straddle, the operator blocks [u(dom) u(bdy) | Lap | dt | div]."""
    import torch
    from scasml_gp_amd import _lib
    lib = _lib.load()
    d, nd, nb = 20, 150, 30
    eq, dom, bdy = _problem(d, nd, nb)
    xd = torch.from_numpy(np.ascontiguousarray(dom, dtype=np.float32)).cuda()
    xb = torch.from_numpy(np.ascontiguousarray(bdy, dtype=np.float32)).cuda()
    M = 4 * nd + nb
    a = 1.0 / (0.25 ** 2 * d)
    K = torch.empty((M, M), dtype=torch.float64, device="cuda")
    _lib.check(lib.scasml_gp_gram(d, a, _lib.ptr(xd), nd, _lib.ptr(xb), nb, _lib.ptr(K), _lib.stream_ptr()), "gp_gram")
    ld = ncols + 5
    out = torch.full((nrows, ld), -7.0, dtype=torch.float64, device="cuda")
    _lib.check(lib.scasml_gp_gram_rows(d, a, _lib.ptr(xd), nd, _lib.ptr(xb), nb, row0, nrows, ncols, _lib.ptr(out), ld, _lib.stream_ptr()), "gp_gram_rows")
    assert torch.equal(out[:, :ncols], K[row0:row0 + nrows, :ncols])
    assert bool((out[:, ncols:] == -7.0).all())                     # nothing beyond the requested columns is touched


@pytest.mark.parametrize("row0,nrows,ncols", [(0, 630, 630), (100, 300, 400), (170, 20, 190), (329, 257, 586), (480, 150, 37), (629, 1, 630)])
def test_compat_gram_rows_equal_the_rows_of_the_as_coded_gram(row0, nrows, ncols):
    """scasml_gp_gram_compat_rows against the same rows of scasml_gp_gram_compat (shifted Hutchinson blocks, float16 entries): bit-identical,
    for ranges that start and end inside, and straddle, the operator blocks."""
    import ctypes as C
    import torch
    from scasml_gp_amd import _lib
    lib = _lib.load()
    d, nd, nb = 20, 150, 30
    eq, dom, bdy = _problem(d, nd, nb)
    xd = torch.from_numpy(np.ascontiguousarray(dom, dtype=np.float32)).cuda()
    xb = torch.from_numpy(np.ascontiguousarray(bdy, dtype=np.float32)).cuda()
    M = 4 * nd + nb
    a = 1.0 / (0.25 ** 2 * d)
    idx = np.asarray([11, 17, 12, 6, 4], dtype=np.int32)
    K = torch.empty((M, M), dtype=torch.float64, device="cuda")
    _lib.check(lib.scasml_gp_gram_compat(d, a, _lib.ptr(xd), nd, _lib.ptr(xb), nb, idx.ctypes.data_as(C.c_void_p), 1, _lib.ptr(K), _lib.stream_ptr()), "gp_gram_compat")
    ld = ncols + 5
    out = torch.full((nrows, ld), -7.0, dtype=torch.float64, device="cuda")
    _lib.check(lib.scasml_gp_gram_compat_rows(d, a, _lib.ptr(xd), nd, _lib.ptr(xb), nb, idx.ctypes.data_as(C.c_void_p), 1, row0, nrows, ncols,
                                              _lib.ptr(out), ld, _lib.stream_ptr()), "gp_gram_compat_rows")
    assert torch.equal(out[:, :ncols], K[row0:row0 + nrows, :ncols])
    assert bool((out[:, ncols:] == -7.0).all())
    assert bool((K.half().double() == K).all())                     # the entries are float16 values (models/GP.py:43, 55-179)


def _worker(rank, world, port, case, q):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), HSA_ENABLE_IPC_MODE_LEGACY="0")
    import torch
    import torch.distributed as dist
    torch.cuda.set_device(0)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from scasml_gp_amd.dist_gp import Comm, DistCholesky, DistributedGP
        from scasml_gp_amd.models.GP import GP_Grad_Dependent_Nonlinear
        if case == "factor":
            d, nd, nb = 250, 8333, 1667                              # M = 34 999: the staged size of BASELINE configs[4]
            eq, dom, bdy = _problem(d, nd, nb)
            gp, L = _single_gpu_factor(eq, dom, bdy)
            ch = DistCholesky(d, 1.0 / float(gp.sigma) ** 2, dom, bdy, gp.nugget, Comm()).build().factor()
            rel = _check_against_single_gpu(ch, L, 1e-10)
            b = torch.from_numpy(np.random.default_rng(0).standard_normal(ch.M)).cuda()
            x = ch.solve(b)
            from scasml_gp_amd import _lib
            lib = _lib.load()
            Mp32 = gp._L_pad.shape[0]
            ref = torch.zeros((Mp32, 1), dtype=torch.float64, device="cuda")
            ref[:ch.M, 0] = b
            _lib.check(lib.scasml_trsm_lower(_lib.ptr(gp._L_pad), Mp32, _lib.ptr(ref), 1, 0, _lib.stream_ptr()), "trsm")
            _lib.check(lib.scasml_trsm_lower(_lib.ptr(gp._L_pad), Mp32, _lib.ptr(ref), 1, 1, _lib.stream_ptr()), "trsm")
            err = float((x - ref[:ch.M, 0]).abs().max() / ref.abs().max())
            q.put((rank, rel, err, ch.memory_bytes(), ch.comm.bytes_moved))
        elif case == "fit_compat":
            d, nd, nb = 20, 1600, 601                                # M = 7001, 28 block rows over 2 ranks
            eq, dom, bdy = _problem(d, nd, nb)
            one = GP_Grad_Dependent_Nonlinear(eq)                     # the default: the reference's as-coded surrogate
            one.GPsolver(dom, bdy, GN_steps=20)
            gp = GP_Grad_Dependent_Nonlinear(eq)
            fit = DistributedGP(gp, Comm())
            fit.fit(dom, bdy, GN_steps=20)
            assert gp.compat == "reference" and fit.chol.round_diag and fit.chol.compat_idx is not None
            rv_err = float(np.abs(gp.right_vector - one.right_vector).max() / np.abs(one.right_vector).max())
            X = np.concatenate(eq.generate_test_data(200, 40))
            pred_err = float(np.abs(gp.predict(X).astype(np.float64) - one.predict(X).astype(np.float64)).max())
            q.put((rank, rv_err, pred_err, len(gp.loss_history) - len(one.loss_history),
                   float(abs(gp.loss_history[-1] - one.loss_history[-1]) / one.loss_history[-1]), max(fit.cg_iterations)))
        elif case == "indefinite":
            d, nd, nb = 20, 150, 30                                  # M = 630, 3 block rows over 2 ranks: the LAST one belongs to rank 0
            eq, dom, bdy = _problem(d, nd, nb)
            ch = DistCholesky(d, 1.0 / 5.0, dom, bdy, 1e-2, Comm()).build()
            last = ch.nblk - 1
            if last in ch.mine:                                      # make the last diagonal block indefinite on its owner only
                slot = ch.mine.index(last)
                ch.R[slot * 256 + 3, last * 256 + 3] = -50.0
            try:
                ch.factor()
                q.put((rank, "no error"))
            except ValueError as e:
                q.put((rank, "ValueError: " + str(e)))
        else:
            d, nd, nb = 20, 350, 70                                  # M = 1470, 6 block rows over 3 ranks
            eq, dom, bdy = _problem(d, nd, nb)
            one = GP_Grad_Dependent_Nonlinear(eq, compat=None)
            one.GPsolver(dom, bdy, GN_steps=20)
            gp = GP_Grad_Dependent_Nonlinear(eq, compat=None)
            fit = DistributedGP(gp, Comm())
            fit.fit(dom, bdy, GN_steps=20)
            rv_err = float(np.abs(gp.right_vector - one.right_vector).max() / np.abs(one.right_vector).max())
            X = np.concatenate(eq.generate_test_data(200, 40))
            pred_err = float(np.abs(gp.predict(X) - one.predict(X)).max())
            q.put((rank, rv_err, pred_err, len(gp.loss_history) - len(one.loss_history),
                   float(abs(gp.loss_history[-1] - one.loss_history[-1]) / one.loss_history[-1]), max(fit.cg_iterations)))
    finally:
        dist.destroy_process_group()


def _worker_rccl(rank, world, port, case, q):
    """ONE rank under init_process_group("nccl") (RCCL on ROCm) with Comm(force=True): at world == 1 every collective is a copy onto itself,
    but it is issued through RCCL on device tensors -- from the side stream and the main stream of the look-ahead factorisation -- which is
    the part of the distributed GP a one-GPU box can execute."""
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), HSA_ENABLE_IPC_MODE_LEGACY="0")
    import torch
    import torch.distributed as dist
    torch.cuda.set_device(0)
    dist.init_process_group("nccl", rank=0, world_size=1, device_id=torch.device("cuda", 0))
    try:
        from scasml_gp_amd.dist_gp import Comm, DistCholesky, DistributedGP
        from scasml_gp_amd.models.GP import GP_Grad_Dependent_Nonlinear
        d, nd, nb = 20, 1600, 601                                    # M = 7001, 28 block rows
        eq, dom, bdy = _problem(d, nd, nb)
        one = GP_Grad_Dependent_Nonlinear(eq)
        one.GPsolver(dom, bdy, GN_steps=20)
        cm = Comm(force=True)
        assert cm.backend == "nccl" and cm.active and not cm.host and cm.world == 1
        a = 1.0 / float(one.sigma) ** 2
        ahead = DistCholesky(d, a, dom, bdy, one.nugget, cm, compat_idx=one.laplacian_idx).build().factor(lookahead=True)
        calls_factor = dict(cm.calls)
        plain = DistCholesky(d, a, dom, bdy, one.nugget, Comm(force=False), compat_idx=one.laplacian_idx).build().factor(lookahead=False)
        torch.cuda.synchronize()
        same = bool(torch.equal(ahead.R, plain.R))                   # collectives through RCCL on two streams vs none at all: the same factor
        b = torch.from_numpy(np.random.default_rng(0).standard_normal(ahead.M)).cuda()
        same = same and bool(torch.equal(ahead.solve(b), plain.solve(b)))
        mv = plain.matvec(b)                                          # the transposed sweep adds its row groups in fixed order: bit for bit,
        same = same and bool(torch.equal(ahead.matvec(b), mv)) and bool(torch.equal(plain.matvec(b), mv))   # between the two objects and between two calls
        del ahead, plain
        gp = GP_Grad_Dependent_Nonlinear(eq)
        fit = DistributedGP(gp, cm)
        fit.fit(dom, bdy, GN_steps=20)
        rv_err = float(np.abs(gp.right_vector - one.right_vector).max() / np.abs(one.right_vector).max())
        X = np.concatenate(eq.generate_test_data(200, 40))
        pred_err = float(np.abs(gp.predict(X).astype(np.float64) - one.predict(X).astype(np.float64)).max())
        q.put((0, cm.backend, same, calls_factor, dict(cm.calls), rv_err, pred_err, len(gp.loss_history) - len(one.loss_history)))
    finally:
        dist.destroy_process_group()


def _run(world, case, timeout, worker=None):
    """One result per rank, sorted; the launcher (tests/_dist_ranks.py) leaves no rank alive, whatever happens."""
    from _dist_ranks import run_ranks
    return run_ranks(world, worker or _worker, (case,), timeout)


def test_two_ranks_factor_M35k_to_the_single_gpu_factor():
    """a 2-rank run sharing one GPU factors M ~ 35k to the single-GPU factor within 1e-10."""
    res = _run(2, "factor", 900)
    for rank, rel, err, mem, moved in res:
        assert rel <= 1e-10 and err <= 1e-9, res
        assert mem == 69 * 256 * 35072 * 8 or mem == 68 * 256 * 35072 * 8      # 137 block rows over 2 ranks
        assert moved > 0.4 * 35072 * 35072 * 8 / 2                              # the column panels reach every rank once


def test_three_ranks_newton_cg_fit_matches_the_single_gpu_fit():
    """Matrix-free Newton with preconditioned CG on the distributed factor against the dense Newton of the single-GPU path:
    the same iterates (same number of steps, loss to 1e-9, right_vector to 1e-6) in a few dozen products per step."""
    res = _run(3, "fit", 900)
    for rank, rv_err, pred_err, dsteps, dloss, cg_max in res:
        assert rv_err <= 1e-6 and pred_err <= 2e-5 and dsteps == 0 and dloss <= 1e-9, res
        assert cg_max <= 150, res


def test_two_ranks_fit_the_as_coded_surrogate_to_the_single_gpu_fit():
    """configs[4] must run the estimator every other configuration runs.  Two ranks build the Gram AS CODED by the reference
    block row by block row (float16 entries, shifted Hutchinson blocks), run the matrix-free Newton on its factor, then round z4 and the diagonal of
    K + nugget I to float16 and solve the rounded matrix with a second distributed factorisation (models/GP.py:268, 599, 719): right_vector of the
    single-GPU compat="reference" fit to 1e-6 at M = 7001; predictions (float16 values) within an ulp."""
    res = _run(2, "fit_compat", 900)
    for rank, rv_err, pred_err, dsteps, dloss, cg_max in res:
        assert rv_err <= 1e-6 and pred_err <= 2.0 ** -10 and dsteps == 0 and dloss <= 1e-8, res


def test_a_failed_pivot_on_one_rank_raises_on_every_rank():
    """scasml_cholesky resets its status word per call and only the owner of a diagonal block sees its pivot fail; the
    status is accumulated over the blocks and all-reduced once, so both ranks raise (instead of one leaving the other in a collective)."""
    res = _run(2, "indefinite", 300)
    assert len(res) == 2 and all(msg.startswith("ValueError") and "not positive definite" in msg for _, msg in res), res


def test_one_rank_under_rccl_issues_every_collective_of_the_distributed_fit():
    """init_process_group("nccl") with one rank in a fresh child process, Comm(force=True): broadcast, all_reduce and
    all_gather_into_tensor run through RCCL on device tensors from both streams of the look-ahead factorisation; the factor, the solves and
    the as-coded Newton-CG fit (M = 7001) equal the collective-free / single-GPU results."""
    (_, backend, same, calls_factor, calls, rv_err, pred_err, dsteps), = _run(1, "rccl", 900, worker=_worker_rccl)
    assert backend == "nccl" and same
    assert calls_factor["broadcast"] == 28 and calls_factor["all_gather"] == 27 and calls_factor["all_reduce"] == 1, calls_factor
    # the substitutions of every CG product: 2 x 7 group steps (four block rows each) per solve, one all-reduce each -- no broadcast beyond the factorisations'
    assert calls["all_reduce"] > 1000 and calls["broadcast"] == 3 * 28, calls      # (three factorisations went through this Comm)
    assert rv_err <= 1e-6 and pred_err <= 2.0 ** -10 and dsteps == 0, (rv_err, pred_err, dsteps)


def test_inexact_newton_reaches_the_same_fit_in_fewer_products():
    """DistributedGP.fit(cg_tol="adaptive"): the inner CG tolerance follows the gradient norm (Eisenstat-Walker forcing term) -- the minimiser the
    dense Newton of the single-GPU path reaches, to the accuracy of the reference's own stopping rule (|grad| < 1e-5, models/GP.py:521), in a
    fraction of the operator products.  World = 1 in process, the as-coded surrogate."""
    from scasml_gp_amd.dist_gp import DistributedGP
    from scasml_gp_amd.models.GP import GP_Grad_Dependent_Nonlinear
    eq, dom, bdy = _problem(20, 700, 140)                          # M = 2940
    one = GP_Grad_Dependent_Nonlinear(eq)
    one.GPsolver(dom, bdy, GN_steps=20)
    tight, loose = GP_Grad_Dependent_Nonlinear(eq), GP_Grad_Dependent_Nonlinear(eq)
    f_tight, f_loose = DistributedGP(tight), DistributedGP(loose)
    f_tight.fit(dom, bdy, GN_steps=20)
    f_loose.fit(dom, bdy, GN_steps=20, cg_tol="adaptive")
    assert np.abs(tight.right_vector - one.right_vector).max() <= 1e-6 * np.abs(one.right_vector).max()
    assert sum(f_loose.cg_iterations) < 0.6 * sum(f_tight.cg_iterations), (f_loose.cg_iterations, f_tight.cg_iterations)
    assert loose.grad_norms[-1] < 1e-5 or len(loose.loss_history) == 21
    assert abs(loose.loss_history[-1] - one.loss_history[-1]) <= 1e-7 * one.loss_history[-1]
    # right_vector: NOT the dense path's to the last digits -- z4 = float16(time_der_rep(sol)) (models/GP.py:719) rounds a few entries the
    # other way for a sol that differs in the eighth digit, and K_p^-1 amplifies those ulps (measured 3.2e-3 here and at M = 70 001); bounded, so
    # that a regression of the forcing term shows, and the predictions below stay within one float16 ulp
    rel = np.abs(loose.right_vector - one.right_vector).max() / np.abs(one.right_vector).max()
    assert 1e-12 < rel <= 1e-2, rel
    X = np.concatenate(eq.generate_test_data(200, 40))
    assert np.abs(loose.predict(X).astype(np.float64) - one.predict(X).astype(np.float64)).max() <= 2.0 ** -10      # float16 values: within an ulp
