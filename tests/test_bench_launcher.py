"""CPU: `python bench.py --gpus N` without a launcher starts N ranks of itself (fresh child processes, parent only
collects) - the N-rank rendezvous, barrier and reductions run here over gloo with world size 2, no GPU, no engine."""
import json
import os
import subprocess
import sys

import pytest

from tests import _harness as H


def _run(args, env_extra=None, drop=("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_PORT")):
    env = {k: v for k, v in os.environ.items() if k not in drop}
    env.update(env_extra or {})
    r = subprocess.run([sys.executable, os.path.join(H.ROOT, "bench.py")] + args, capture_output=True, text=True, env=env,
                       timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout
    return json.loads(lines[0])


def test_self_launch_two_ranks():
    d = _run(["--gpus", "2", "--launch-check"])
    assert d["launch_check"] and d["n_gpus"] == 2
    assert d["streams_total"] == 2 * 65536           # SUM over ranks of the contiguous shards = the whole job
    assert abs(d["max_time"] - 0.002) < 1e-12        # MAX over ranks
    assert d["per_rank_streams"] == [65536.0, 65536.0]       # every rank's own figure, gathered


def test_single_rank_needs_no_rendezvous():
    d = _run(["--gpus", "1", "--launch-check"])
    assert d["n_gpus"] == 1 and d["streams_total"] == 65536


def test_under_an_external_launcher_nothing_is_spawned():
    """With WORLD_SIZE in the environment (torch.distributed.run) the script is a rank, not a launcher."""
    d = _run(["--gpus", "2", "--launch-check"], env_extra={"WORLD_SIZE": "1", "RANK": "0", "LOCAL_RANK": "0"}, drop=())
    assert d["n_gpus"] == 1


def test_eight_ranks_plan_the_8m_stream_job():
    """BASELINE configs[4]: 8M streams over 8 ranks.  Eight gloo ranks (CPU) rendezvous, take their contiguous shards and
    plan the HBM of their share of the transcode (sharding.plan_transcode_bytes: I/O and per-stream state grow with the
    shard, the engine's workspaces stop at ac3mi_set_tile_frames' default): every rank fits 288 GB with room to spare."""
    d = _run(["--gpus", "8", "--launch-check", "--job-streams", str(8 * (1 << 20))])
    assert d["n_gpus"] == 8 and d["streams_total"] == 8 * (1 << 20)
    assert d["ranks_that_fit_288GB"] == 8
    assert 20e9 < d["max_rank_hbm_plan_bytes"] < 60e9


@pytest.mark.gpu
def test_two_rank_line_carries_every_ranks_rate_and_the_cpu_baseline():
    """The N-rank code path of the real bench on the one-GPU box: both ranks on device 0 over gloo (AC3MI_BENCH_REHEARSE=1;
    RCCL refuses two ranks on one device).  The line must name BASELINE's metric, carry one rate per rank - a slow GPU
    cannot hide behind the MAX-reduced time - and keep its cpu_baseline (rank 0 measures it after the barrier)."""
    d = _run(["--gpus", "2", "--steps", "2", "--warmup", "1", "--frames", "2048", "--no-extra"],
             env_extra={"AC3MI_BENCH_REHEARSE": "1", "AC3MI_BENCH_MILLION": "0"})
    assert d["n_gpus"] == 2 and d["metric"] == json.load(open(os.path.join(H.ROOT, "BASELINE.json")))["metric"]
    assert len(d["per_rank_frames_per_s"]) == 2 and all(x > 0 for x in d["per_rank_frames_per_s"])
    assert abs(d["value"] - 2 * 2048 * 2 / (d["ms_per_step"] * 2e-3)) < 1e-6 * d["value"]
    assert d["all_frames_ok"] and d["cpu_baseline"] and d["cpu_baseline"]["value"] > 0
    assert d["roofline"]["hbm"]["frac"] > 0


@pytest.mark.gpu
def test_dump_outputs_hold_the_last_steps_results(tmp_path):
    """--dump-outputs DIR: what the timed transcode handed back in its last step, for a seeded sample of the streams, as
    float32 / float64 .npy files of 64 MB at most.  Every step starts from fresh stream state, so two runs with different
    step counts must dump the same arrays; the frames must be valid AC-3 (both CRCs) and the decode status clean."""
    import numpy as np
    import bench
    dumps = []
    for steps in (2, 3):
        out = tmp_path / ("s%d" % steps)
        d = _run(["--gpus", "1", "--steps", str(steps), "--warmup", "1", "--frames", "4096", "--no-extra", "--no-cpu-baseline",
                  "--dump-outputs", str(out)], env_extra={"AC3MI_BENCH_MILLION": "0"})
        assert d["steps"] == steps and d["ms_per_step"] > 0 and d["all_frames_ok"]
        assert d["dump_outputs"]["streams"] == 2048
        dumps.append({n: np.load(str(out / (n + ".npy"))) for n in d["dump_outputs"]["arrays"]})
    a, b = dumps
    assert sorted(a) == ["csnroffst", "delay", "frames", "last_samples", "lfsr", "status", "stream_index"]
    assert all(x.dtype in (np.float32, np.float64) for x in a.values())
    assert sum(x.nbytes for x in a.values()) <= 64 << 20
    for n in a:
        assert np.array_equal(a[n], b[n]), n
    idx = a["stream_index"]
    assert idx.size == 2048 and np.all(np.diff(idx) > 0) and 0 <= idx[0] and idx[-1] < 4096
    frames = a["frames"].reshape(2048, -1)
    assert np.array_equal(frames, np.round(frames)) and frames.min() >= 0 and frames.max() <= 255
    assert bench.ac3_crc_ok(frames.astype(np.uint8)) == 0
    assert (a["status"].astype(np.int64) & 0x1ff).max() == 0
