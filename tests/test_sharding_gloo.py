"""CPU, world_size 2 over gloo: the N>1 layout used by bench.py - contiguous stream shards, no
data-path collective, MAX-reduced timing, SUM-reduced frame counts."""
import os
import socket

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from tests import _harness as H


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _worker(rank, world, port, n_streams, q):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world),
                      LOCAL_RANK=str(rank))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    sh = H.pkg().sharding
    lo, hi = sh.shard(n_streams, world, rank)
    # each rank "processes" its own streams: here the CPU oracle transform on a tiny batch
    rng = np.random.default_rng(1234)
    coef = (rng.standard_normal((n_streams, 1, 6, 6, 256)) * 0.05).astype(np.float32)
    pcm, _ = H.orc_xform(coef[lo:hi], None, 7, 1, 7 | 16)
    t = 0.010 * (rank + 1)
    tmax, = sh.reduce_max([t], dist)
    total, = sh.reduce_sum([hi - lo], dist)
    dist.barrier()
    q.put((rank, lo, hi, tmax, total, float(np.abs(pcm).sum())))
    dist.destroy_process_group()


def test_shards_cover_all_streams_without_overlap():
    sh = H.pkg().sharding
    for n in (0, 1, 7, 8, 65536, 8_000_000, 8_000_003):
        for world in (1, 2, 3, 4, 8):
            spans = [sh.shard(n, world, r) for r in range(world)]
            assert spans[0][0] == 0 and spans[-1][1] == n
            assert all(a[1] == b[0] for a, b in zip(spans, spans[1:]))
            sizes = [b - a for a, b in spans]
            assert max(sizes) - min(sizes) <= 1


def test_two_ranks_gloo():
    import importlib
    H.pkg()                                       # make sure the package (and .sharding) imports in the parent
    importlib.import_module("ac-3-acm-codec_amd.sharding")
    world, n_streams = 2, 5
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, world, port, n_streams, q)) for r in range(world)]
    for p in procs:
        p.start()
    res = sorted(q.get(timeout=120) for _ in procs)
    for p in procs:
        p.join(60)
        assert p.exitcode == 0
    assert [(r[1], r[2]) for r in res] == [(0, 3), (3, 5)]
    assert all(abs(r[3] - 0.020) < 1e-12 for r in res)          # MAX over ranks
    assert all(r[4] == n_streams for r in res)                  # SUM of per-rank work = whole job
    # sharded result == unsharded result (streams are independent)
    rng = np.random.default_rng(1234)
    coef = (rng.standard_normal((n_streams, 1, 6, 6, 256)) * 0.05).astype(np.float32)
    pcm, _ = H.orc_xform(coef, None, 7, 1, 7 | 16)
    assert abs(sum(r[5] for r in res) - float(np.abs(pcm).sum())) < 1e-3


def test_rank_plan_fits_hbm():
    """What one rank plans for its shard (sharding.plan_transcode_bytes): the workspaces stop growing at the tile bound,
    so BASELINE configs[4]'s per-GPU share (2^20 streams) needs ~25 GB, and a rank could hold about 25 M one-frame streams."""
    sh = H.pkg().sharding
    lo, hi = sh.shard(8 * (1 << 20), 8, 5)
    p = sh.plan_transcode_bytes(hi - lo)
    assert p["fits"] and 20e9 < p["total"] < 60e9
    assert p["workspace"] == sh.plan_transcode_bytes(1 << 24)["workspace"]           # bounded by the tile
    assert sh.plan_transcode_bytes(4096)["workspace"] < p["workspace"]                # small batches: only what they use
    assert not sh.plan_transcode_bytes(40_000_000)["fits"]
    # one-frame streams decode through the fused mantissa + transform kernel: no coefficient planes (6 blocks x 6 planes x 256
    # floats per frame) in the workspace; streams of several frames keep them
    one = sh.plan_transcode_bytes(65536, frames_per_stream=1)["workspace"]
    two = sh.plan_transcode_bytes(32768, frames_per_stream=2)["workspace"]
    assert two - one == 65536 * 6 * 6 * 256 * 4


@pytest.mark.parametrize("args, want", [
    ((131072, 1, 6, 5, 6), 13_372_360_452),
    ((131072, 4, 6, 5, 6), 18_204_198_660),
    ((4096, 1, 2, 2, 2), 205_281_028),
    ((6000, 3, 6, 5, 2), 521_998_484),
    ((100, 1, 6, 5, 2), 8_702_880),
    ((7, 2, 3, 2, 2), 484_095),
])
def test_transcode_workspace_plan_is_pinned(args, want):
    """ac3mi_transcode_workspace_plan(frames, frames_per_stream, n_in, nfchans, n_out), no GPU: the bytes the transcode's
    allocation expressions give, pinned - with and without coefficient planes, several frames a stream, a downmix."""
    import ctypes
    lib = H.pkg().load_library()
    f = lib.ac3mi_transcode_workspace_plan
    f.restype = ctypes.c_size_t
    f.argtypes = [ctypes.c_size_t, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int]
    assert f(*args) == want
