"""``parallel.solve_sharded(..., return_stderr=...)``: the standard errors of a sharded solve (scasml_gp_amd/parallel.py).

Without a process group the call is the solver's own fused estimate on the same stream; with one, ``mode="samples"`` all-reduces every rank's
table of summands together with its partial sums and closes the variance from the completed table (tests/test_gpu_picard_summands.py holds
that table and the closed estimate against the oracle), and ``mode="roots"`` gathers the fused estimate of every rank's slice.  The 2-rank
run shares GPU 0 over gloo, set up as the ranks of tests/test_gpu_dist_gp.py are."""
import os

import numpy as np
import pytest

from test_gpu_picard_stderr import _mlp, _points, _same_bits, _scasml, _scasml_points, _solve

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("variant,n,par", [("quad", 3, 3), ("fh", 2, 3)])
@pytest.mark.parametrize("mode", ["samples", "roots"])
def test_without_a_process_group_it_is_the_solvers_own_estimate(variant, n, par, mode):
    from scasml_gp_amd import parallel
    hip, _ = _mlp(20, variant, seed=5)
    eng = hip._engine
    xt = _points(20, 9, 40)
    for flag in (True, "uz"):
        eng.calls = 3
        want_uz, want_se = _solve(hip, variant, n, par, xt, return_stderr=flag)
        assert eng.calls == 4
        eng.calls = 3
        uz, se = parallel.solve_sharded(hip, n, par, xt, mode=mode, return_stderr=flag)
        assert eng.calls == 4 and _same_bits(uz, want_uz) and _same_bits(se, want_se)
        assert tuple(se.shape) == ((9, 1) if flag is True else (9, 21))
    # return_stderr=False: what the call has always returned, on the stream it has always used
    eng.calls = 3
    plain = _solve(hip, variant, n, par, xt)
    eng.calls = 3
    assert _same_bits(parallel.solve_sharded(hip, n, par, xt, mode=mode), plain) and eng.calls == 4
    assert _same_bits(plain, want_uz)


def test_refusals_of_the_estimate_hold_and_move_no_counter():
    from scasml_gp_amd import _lib, parallel
    from scasml_gp_amd.equations.equations import Grad_Dependent_Nonlinear
    from scasml_gp_amd.solvers.MLP import MLP
    xt = _points(20, 4, 5)
    eq = Grad_Dependent_Nonlinear(21)
    for mode in ("samples", "roots"):
        hip = MLP(eq)
        with pytest.raises(ValueError, match="no estimable variance"):
            parallel.solve_sharded(hip, 2, 2, xt, mode=mode, return_stderr=True)
        assert hip._engine.calls == 0
        crn = MLP(eq, compat_crn=True)
        with pytest.raises(_lib.ScasmlError):
            parallel.solve_sharded(crn, 3, 3, xt, mode=mode, return_stderr="uz")
        assert crn._engine.calls == 0
    with pytest.raises(ValueError, match="mode"):
        parallel.solve_sharded(MLP(eq), 3, 3, xt, mode="paths", return_stderr=True)


def _in_turn(eng, n, par, xt, world, form, chunk=None):
    """What ``world`` ranks of a sample-sharded solve compute, launched in turn in this process: per root chunk the ranks' flat buffers
    (partial sums, then the table) added in rank order as an all-reduce adds them, the sums clipped, the variance closed from the table."""
    import torch
    from scasml_gp_amd import parallel
    B, d = xt.shape[0], xt.shape[1] - 1
    ncol, S = (d + 1 if form == "uz" else 1), eng.root_summands(n, par)
    chunk = chunk or B
    uz = torch.empty((B, d + 1), dtype=torch.float32, device="cuda")
    se = torch.empty((B, ncol), dtype=torch.float32, device="cuda")
    for b0 in range(0, B, chunk):
        nb = min(chunk, B - b0)
        flats = [torch.empty((nb * (d + 1) + S * nb * ncol,), dtype=torch.float32, device="cuda") for _ in range(world)]
        for r in range(world):
            eng.solve(n, par, xt[b0:b0 + nb], root0=b0, rank=r, world=world, stream_id=0, summands=form, buffer=flats[r])
        acc = flats[0].clone()
        for f in flats[1:]:
            acc += f
        uz[b0:b0 + nb] = eng.finalize_partials(acc[:nb * (d + 1)].view(nb, d + 1))
        se[b0:b0 + nb] = eng.finalize_summands(acc[nb * (d + 1):].view(S, nb, ncol), n, par)
    return uz, se


def test_root_chunks_of_the_summand_buffer_return_the_unchunked_bits(monkeypatch):
    """MLP mode: a root's walk depends on its global index alone, so walking the batch three roots at a time (each chunk with root0 = its
    offset and its own reduction) changes no bit.  The chunking is that of parallel._samples_with_stderr, reached here through its helper
    at world = 2 with the ranks in turn."""
    from scasml_gp_amd import parallel
    hip, _ = _mlp(20, "quad", seed=5)
    eng = hip._engine
    xt = _points(20, 8, 40)
    S = eng.root_summands(3, 3)
    for form, ncol in (("u", 1), ("uz", 21)):
        whole = _in_turn(eng, 3, 3, xt, 2, form)
        monkeypatch.setattr(parallel, "SUMMAND_BUFFER_BYTES", 4 * S * ncol * 3)
        calls = []
        monkeypatch.setattr(parallel, "allreduce_partial_sums", lambda flat, group=None: calls.append(flat.numel()) or flat)
        uz, se = parallel._samples_with_stderr(eng, 3, 3, xt, 0, 1, 0, form == "uz", None)      # one rank owning everything: the chunk walk itself
        assert calls == [3 * (21 + S * ncol)] * 2 + [2 * (21 + S * ncol)]                          # 3 + 3 + 2 roots, one reduction each
        monkeypatch.undo()
        one = _in_turn(eng, 3, 3, xt, 1, form)
        assert _same_bits(uz, one[0]) and _same_bits(se, one[1])
        three = _in_turn(eng, 3, 3, xt, 2, form, chunk=3)
        assert _same_bits(three[0], whole[0]) and _same_bits(three[1], whole[1])


def _rank(rank, world, port, q):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), HSA_ENABLE_IPC_MODE_LEGACY="0")
    import torch
    import torch.distributed as dist
    torch.cuda.set_device(0)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from scasml_gp_amd import parallel
        hip, _ = _mlp(20, "quad", seed=5)
        xt = _points(20, 9, 40)
        out = []
        for mode in ("samples", "roots"):
            hip._engine.calls = 0
            uz, se = parallel.solve_sharded(hip, 3, 3, xt, mode=mode, return_stderr="uz")
            out += [uz.cpu().numpy(), se.cpu().numpy()]
        hip._engine.calls = 0
        uz, se = parallel.solve_sharded(hip, 3, 3, xt, mode="samples", return_stderr=True)
        out += [uz.cpu().numpy(), se.cpu().numpy(), hip._engine.calls]
        q.put((rank, out))
    finally:
        dist.destroy_process_group()


def test_two_ranks_return_identical_results_equal_to_the_in_turn_ones():
    from _dist_ranks import run_ranks
    (r0, a), (r1, b) = run_ranks(2, _rank, (), 300)
    assert (r0, r1) == (0, 1) and a[-1] == b[-1] == 1
    for x, y in zip(a[:-1], b[:-1]):
        assert _same_bits(x, y)
    hip, _ = _mlp(20, "quad", seed=5)
    eng = hip._engine
    xt = _points(20, 9, 40)
    uz, se = _in_turn(eng, 3, 3, xt, 2, "uz")
    assert _same_bits(a[0], uz) and _same_bits(a[1], se)
    uz_u, se_u = _in_turn(eng, 3, 3, xt, 2, "u")
    assert _same_bits(a[4], uz_u) and _same_bits(a[5], se_u) and se_u.shape == (9, 1)
    # roots: every rank's slice is the fused estimate of those roots, whatever the rank count
    eng.calls = 0
    want_uz, want_se = hip.uz_solve(3, 3, xt, return_stderr="uz")
    assert _same_bits(a[2], want_uz) and _same_bits(a[3], want_se)
