"""Multi-GPU host logic: one process per GPU, torch.distributed (backend "nccl" = RCCL on ROCm;
"gloo" in the CPU tests).

Two shardings of the Picard solve:

* ``roots``   -- evaluation points are independent; each rank solves a contiguous slice with
                 ``root0`` = its global offset (Philox counters are keyed by the GLOBAL root index,
                 so the result does not depend on the rank count).  No data-path collective; an
                 optional all_gather returns the full result everywhere.  This is what bench.py uses.
* ``samples`` -- the Monte-Carlo units of the ROOT call (terminal samples, then per node (m, k) of every
                 level's sample paths its "+" and "-" addends with their subtrees) are dealt to ranks by cost
                 (scasml_plan_deal_units); each rank produces un-clipped partial sums of shape (B, 1+d) and ONE
                 all-reduce(sum) over xGMI combines them, followed by the clip of MLP.py:272-274.  The reference
                 has no counterpart (single device).  With ``return_stderr`` every rank also stores its partial of every
                 root-call summand into a table (scasml_picard_tree_summands) that travels in the SAME all-reduce, and a small
                 kernel closes the variance from the completed table: 4 S B bytes more for the error of u, 4 S B (1 + d) for
                 those of (u, z) -- at the headline shape (S = 37, 16384 roots, d = 100) 2.4 MB and 245 MB against 6.6 MB of
                 partial sums.
"""

# cap on one all-reduce buffer's table of summands (bytes): beyond it a sample-sharded solve with standard errors walks the batch in root
# chunks, each with its own all-reduce
SUMMAND_BUFFER_BYTES = 1 << 30


def root_slice(total, rank, world):
    """Contiguous split of ``total`` roots: (start, count) for ``rank``; earlier ranks take the remainder."""
    base, rem = divmod(int(total), int(world))
    count = base + (1 if rank < rem else 0)
    start = rank * base + min(rank, rem)
    return start, count


def sample_units(plan):
    """Number of shardable units of the root call: terminal samples + the addends of the NODES (l, m, k) of every level's sample paths
    ("+" with the level-l subtree; "-" with the level-(l-1) subtree where l > 0)."""
    n = plan.n
    return int(plan.mg[n]) + sum(int(plan.term[n][l].mc) * int(plan.term[n][l].q) * (2 if l else 1) for l in range(n))


def allreduce_partial_sums(partial, group=None):
    """Sum the ranks' partial (B, 1+d) estimators in place -- the single collective of the path."""
    import torch.distributed as dist
    if dist.is_available() and dist.is_initialized() and dist.get_world_size(group) > 1:
        if partial.is_cuda and dist.get_backend(group) == "gloo":     # gloo reduces host memory: the rehearsal of several ranks on one GPU
            host = partial.cpu()
            dist.all_reduce(host, op=dist.ReduceOp.SUM, group=group)
            partial.copy_(host)
        else:
            dist.all_reduce(partial, op=dist.ReduceOp.SUM, group=group)
    return partial


def gather_roots(local, counts, group=None):
    """all_gather root-sharded results (ragged first dimension) into the full batch on every rank."""
    import torch
    import torch.distributed as dist
    if not (dist.is_available() and dist.is_initialized()) or dist.get_world_size(group) == 1:
        return local
    mx = max(counts)
    on_host = local.is_cuda and dist.get_backend(group) == "gloo"     # as in allreduce_partial_sums
    pad = torch.zeros((mx,) + tuple(local.shape[1:]), dtype=local.dtype, device="cpu" if on_host else local.device)
    pad[: local.shape[0]] = local
    outs = [torch.empty_like(pad) for _ in counts]
    dist.all_gather(outs, pad, group=group)
    return torch.cat([o[:c] for o, c in zip(outs, counts)], dim=0).to(local.device)


def _samples_with_stderr(eng, n, par, x_t, rank, world, stream_id, se_uz, group):
    """The sample-sharded solve with standard errors at world > 1: per root chunk ONE flat buffer -- the rank's partial (nb, 1 + d) sums, then
    its (S, nb, ncol) table of summands -- one all-reduce of it, then the clip of the sums and the variance from the completed table.  The
    chunking follows from the shapes alone, so every rank walks the same chunks."""
    import torch
    B, d = len(x_t), eng.equation.n_input - 1
    ncol, S = (d + 1 if se_uz else 1), eng.root_summands(n, par)
    chunk = max(1, min(B, SUMMAND_BUFFER_BYTES // max(1, 4 * S * ncol)))
    uz = torch.empty((B, d + 1), dtype=torch.float32, device="cuda")
    se = torch.empty((B, ncol), dtype=torch.float32, device="cuda")
    for b0 in range(0, B, chunk):
        nb = min(chunk, B - b0)
        flat = torch.empty((nb * (d + 1) + S * nb * ncol,), dtype=torch.float32, device="cuda")
        part, _, _, table = eng.solve(n, par, x_t[b0:b0 + nb], root0=b0, rank=rank, world=world, stream_id=stream_id,
                                      summands="uz" if se_uz else "u", buffer=flat)
        allreduce_partial_sums(flat, group)
        uz[b0:b0 + nb] = eng.finalize_partials(part)
        se[b0:b0 + nb] = eng.finalize_summands(table, n, par)
    return uz, se


def solve_sharded(solver, n, par, x_t, mode="roots", group=None, gather=True, return_stderr=False):
    """Run ``solver`` (an MLP / ScaSML object of this package) on the calling rank's share.

    mode="roots":   x_t is the FULL batch on every rank; returns the full (B, 1+d) result if
                    ``gather`` else the local slice.
    mode="samples": every rank holds the full batch and 1/world of the Monte-Carlo units; returns
                    the all-reduced, clipped (B, 1+d) result on every rank.
    return_stderr=True or "uz": (uz, se), se the (B, 1) Monte-Carlo standard error of u or the (B, 1 + d) errors of (u, z) that
                    ``solver.uz_solve(..., return_stderr=...)`` defines, under its refusals (raised before the call counter moves).
                    "roots": every rank runs the fused estimate on its slice and se is gathered like uz.  "samples": one rank runs
                    the fused estimate; more ranks all-reduce their tables of summands with the partial sums (one collective; the
                    batch in root chunks where the table would pass SUMMAND_BUFFER_BYTES) and close the variance from the
                    completed table -- equal to the unsharded estimate to rounding, and "uz" multiplies the collective by S = the
                    number of root-call summands.
    """
    import torch.distributed as dist
    world = dist.get_world_size(group) if dist.is_initialized() else 1
    rank = dist.get_rank(group) if dist.is_initialized() else 0
    eng = solver._engine
    if return_stderr:
        if mode not in ("roots", "samples"):
            raise ValueError("mode must be 'roots' or 'samples'")
        se_uz = isinstance(return_stderr, str) and return_stderr == "uz"
        sharded = mode == "samples" and world > 1
        eng.check_stderr(int(n), int(par), staged_ok=not sharded)
        stream_id = eng.calls
        eng.calls += 1
        if sharded:
            return _samples_with_stderr(eng, int(n), int(par), x_t, rank, world, stream_id, se_uz, group)
        start, count = root_slice(len(x_t), rank, world) if mode == "roots" else (0, len(x_t))
        uz, _, _, se = eng.solve(int(n), int(par), x_t[start:start + count], root0=start, stream_id=stream_id, stderr="uz" if se_uz else True)
        se = se if se_uz else se[:, None]
        if mode == "samples" or not gather:
            return uz, se
        counts = [root_slice(len(x_t), r, world)[1] for r in range(world)]
        return gather_roots(uz, counts, group), gather_roots(se, counts, group)
    stream_id = eng.calls
    eng.calls += 1
    if mode == "roots":
        start, count = root_slice(len(x_t), rank, world)
        uz, _, _ = eng.solve(n, par, x_t[start:start + count], root0=start, stream_id=stream_id)
        if not gather:
            return uz
        return gather_roots(uz, [root_slice(len(x_t), r, world)[1] for r in range(world)], group)
    if mode == "samples":
        uz, _, _ = eng.solve(n, par, x_t, rank=rank, world=world, stream_id=stream_id)
        if world == 1:
            return uz
        return eng.finalize_partials(allreduce_partial_sums(uz, group))
    raise ValueError("mode must be 'roots' or 'samples'")
