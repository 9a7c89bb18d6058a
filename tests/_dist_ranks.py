"""Rank launcher of the distributed tests: ``world`` child processes (spawn context) that share GPU 0 and meet over gloo on a port the
kernel handed out.  Every child reports once through a queue; whatever happens -- a result from everyone, a child that died, the time
limit -- the children still alive are terminated (then killed) BEFORE the caller hears of it, so that no rank is left behind with the
GPU open.  A launch that failed is final for the session: nothing more is started on the GPU after an abort, a segmentation fault or a
hang of a rank (``dead`` below)."""
import os
import queue
import socket
import time

MAX_RANKS = 4                  # children alive at once
ENV = {"MASTER_ADDR": "127.0.0.1", "HSA_ENABLE_IPC_MODE_LEGACY": "0"}      # what the ranks of tests/test_gpu_dist_gp.py set
dead = []                      # why an earlier launch of this session failed (empty: none did)


def free_port():
    """A port nobody listens on: bound to port 0 on the loopback, read back, released."""
    with socket.socket(socket.AF_INET, socket.SOCK_STREAM) as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def rank_env(port):
    """The environment of a rank (a worker applies it with os.environ.update before it imports torch)."""
    return dict(ENV, MASTER_PORT=str(port))


def _entry(target, rank, world, port, args, q):
    os.environ.update(rank_env(port))
    target(rank, world, port, *args, q)


def run_ranks(world, target, args=(), timeout=300.0):
    """Start ``target(rank, world, port, *args, q)`` for rank = 0 .. world - 1 and return the sorted list of what each put on ``q`` (one item
    per rank).  Raises AssertionError -- after every child is gone -- if a child exits with a status other than 0, if a result is missing
    after ``timeout`` seconds, or if an earlier launch of this session failed."""
    import torch.multiprocessing as mp
    assert 1 <= world <= MAX_RANKS, "at most %d ranks share the GPU" % MAX_RANKS
    assert not dead, "not started: an earlier launch failed (%s)" % dead[0]
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = free_port()
    procs = [ctx.Process(target=_entry, args=(target, r, world, port, tuple(args), q)) for r in range(world)]
    res, why = [], None
    try:
        for p in procs:
            p.start()
        limit = time.monotonic() + timeout
        while len(res) < world and why is None:
            try:
                res.append(q.get(timeout=0.5))
                continue
            except queue.Empty:
                pass
            codes = [p.exitcode for p in procs]
            if any(c not in (None, 0) for c in codes):
                why = "a rank ended with exit codes %s" % codes
            elif all(c == 0 for c in codes) and q.empty():
                why = "every rank ended, %d of %d reported" % (len(res), world)
            elif time.monotonic() > limit:
                why = "no result within %g s (exit codes %s)" % (timeout, codes)
        if why is None:
            for p in procs:
                p.join(timeout=120)
            codes = [p.exitcode for p in procs]
            if any(c != 0 for c in codes):
                why = "exit codes %s after the results" % codes
    except BaseException as e:
        why = why or "launcher interrupted: %r" % (e,)
        raise
    finally:
        for p in procs:
            if p.is_alive():
                p.terminate()
        for p in procs:
            if p.pid is not None:
                p.join(timeout=10)
                if p.is_alive():
                    p.kill()
                    p.join(timeout=10)
        if why is not None:
            dead.append(why)
    assert why is None, why
    return sorted(res)
