"""bench.py's multi-rank launch (no GPU): with --gpus N and no launcher it starts N rank processes
itself (RANK / WORLD_SIZE / MASTER_* set, before any HIP call), they rendezvous, and rank 0 reports
the ranks it saw; a WORLD_SIZE that disagrees with --gpus is refused (exit 2) instead of silently
measuring another N."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BENCH = os.path.join(ROOT, "bench.py")


def _env(**kw):
    e = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT")}
    e.update(kw)
    return e


@pytest.mark.parametrize("n", [2, 4])
def test_bench_launches_n_ranks_itself(n):
    r = subprocess.run([sys.executable, BENCH, "--gpus", str(n), "--check-launch"], capture_output=True, text=True,
                       timeout=300, env=_env())
    assert r.returncode == 0, r.stderr[-2000:]
    line = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])
    assert line["ranks_seen"] == n and line["world"] == n


def test_bench_refuses_a_wrong_world_size():
    r = subprocess.run([sys.executable, BENCH, "--gpus", "8", "--check-launch"], capture_output=True, text=True,
                       timeout=120, env=_env(WORLD_SIZE="2", RANK="0", LOCAL_RANK="0", MASTER_ADDR="127.0.0.1",
                                             MASTER_PORT="29512"))
    assert r.returncode == 2
    assert "WORLD_SIZE=2" in r.stderr


def test_bench_launcher_stops_when_a_rank_dies():
    """a rank that dies before the rendezvous must not leave rank 0 waiting for it; the
    launcher kills the others and exits with the failed rank's code."""
    import time
    t0 = time.monotonic()
    r = subprocess.run([sys.executable, BENCH, "--gpus", "2", "--check-launch", "--check-launch-fail-rank", "1"],
                       capture_output=True, text=True, timeout=240, env=_env())
    assert r.returncode == 5, (r.returncode, r.stderr[-2000:])
    assert time.monotonic() - t0 < 200


def test_traffic_only_from_a_profile_of_this_build(tmp_path):
    """roofline.traffic is read from a committed PMC summary only when that summary was
    taken with the libbos.so this process loaded (its sha256); otherwise it is null."""
    sys.path.insert(0, ROOT)
    import bench
    import bos
    bench.bos = bos
    mine = bench.lib_sha256()
    for label, sha in (("instep", mine), ("warm", "0" * 64)):
        with open(tmp_path / f"{bench.PROFILE_TAG}_pmc_linearize_fp32_{label}.json", "w") as f:
            json.dump({"hbm_bytes_per_launch": 123.0, "libbos_sha256": sha}, f)
    t, why = bench.traffic_from_profile(bos.BOS_FP32, str(tmp_path))
    assert t == {"instep": 123.0, "warm": None}
    assert "another libbos.so" in why["warm"]
    t, why = bench.traffic_from_profile(bos.BOS_FP64, str(tmp_path))
    assert t == {"instep": None, "warm": None}


def test_dump_writer_samples_large_arrays_the_same_way_every_time(tmp_path, monkeypatch):
    """--dump-outputs: arrays are written whole as float64 up to the element cap; a larger one is cut
    to a sample of exactly that many elements, the same (ascending) flat indices in every run, and the
    byte limit over all files is enforced."""
    import numpy as np
    sys.path.insert(0, ROOT)
    import bench
    monkeypatch.setattr(bench, "DUMP_MAX_ELEMS", 100)
    small = np.arange(60, dtype=np.float32).reshape(20, 3)
    big = np.arange(1000, dtype=np.float64) * 0.5
    for d in ("a", "b"):
        w = bench.write_outputs(str(tmp_path / d), {"small": small, "big": big})
        assert w == {"small": [60, 60], "big": [100, 1000]}
    a, b = (np.load(tmp_path / d / "big.npy") for d in ("a", "b"))
    assert a.dtype == np.float64 and a.shape == (100,) and np.array_equal(a, b)
    assert np.all(np.diff(a) > 0) and set(a) <= set(big) and not np.array_equal(a, big[:100])
    s = np.load(tmp_path / "a" / "small.npy")
    assert s.dtype == np.float64 and np.array_equal(s, small)
    monkeypatch.setattr(bench, "DUMP_MAX_BYTES", 8 * 150)
    with pytest.raises(RuntimeError, match="--dump-outputs"):
        bench.write_outputs(str(tmp_path / "c"), {"small": small, "big": big})


def test_plain_run_refuses_steps_0():
    """Without --full only the timed GN steps run, so --steps 0 (the J+H builds alone, a --full leg)
    is refused before anything is set up."""
    r = subprocess.run([sys.executable, BENCH, "--gpus", "1", "--steps", "0", "--warmup", "0"], capture_output=True,
                       text=True, timeout=120, env=_env())
    assert r.returncode == 2 and "--full" in r.stderr


@pytest.mark.gpu
def test_plain_c2_run_dumps_the_same_outputs_twice(tmp_path):
    """A plain run (config 2, the small world) prints ms_per_step as the wall time of one timed step,
    leaves the --full keys out, and --dump-outputs writes the last timed step's results: float64,
    finite, of the world's sizes, and equal bit for bit between two runs with the same arguments."""
    import numpy as np
    runs = []
    for d in ("a", "b"):
        r = subprocess.run([sys.executable, BENCH, "--gpus", "1", "--steps", "7", "--warmup", "2", "--config", "c2",
                            "--dump-outputs", str(tmp_path / d)], capture_output=True, text=True, timeout=120,
                           env=_env())
        assert r.returncode == 0, r.stderr[-2000:]
        line = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])
        assert line["steps"] == 7 and line["full"] is False and "cpu_baseline_gn" not in line
        assert abs(line["ms_per_step"] * 1e3 - line["gn_us_per_iteration"]) < 1e-6
        assert line["value"] > 0 and 0 < line["jh_ms_per_step"] < line["ms_per_step"]
        runs.append({f[:-4]: np.load(tmp_path / d / f) for f in sorted(os.listdir(tmp_path / d))})
    a, b = runs
    n = 3 * 1000 + 2 * 2000
    assert {k: v.shape for k, v in a.items() if k != "H_lower_values"} == {
        "pose_xyt": (1000, 3), "landmark_xy": (2000, 2), "chi2": (7,), "n_robust": (7,), "max_abs_dx": (7,),
        "dx": (n,), "b": (n,)}
    assert a["H_lower_values"].ndim == 1 and a["H_lower_values"].size > 20000
    assert sum(v.nbytes for v in a.values()) <= 64 << 20
    for k in a:
        assert a[k].dtype == np.float64 and np.all(np.isfinite(a[k])), k
        assert np.array_equal(a[k], b[k]), k
    assert a["chi2"][-1] < a["chi2"][0] and np.any(a["dx"] != 0)


LADDER_CASES = [
    # (world, failures, expected mode, expected failed attempts)
    (2, "", "p2p", []),
    (2, "p2p:setup@1", "rccl", ["p2p"]),
    (2, "p2p:run@0,rccl:setup@*", "gloo", ["p2p", "rccl"]),
    (8, "p2p:run@5", "rccl", ["p2p"]),
    (8, "p2p:setup@3,rccl:run@7", "gloo", ["p2p", "rccl"]),
    (8, "p2p:setup@*,rccl:run@1,gloo:run@6", None, ["p2p", "rccl", "gloo"]),
]


@pytest.mark.parametrize("world,fails,mode,failed", LADDER_CASES)
def test_exchange_ladder_every_rank_takes_the_same_decision(world, fails, mode, failed):
    """the N > 1 bench falls back p2p -> RCCL -> gloo host exchange when a mode
    fails on any rank (at setup or in its run), every rank agreeing on each step (gloo collectives),
    and rank 0 prints a line whatever fails, naming the failing ranks' reasons. The stand-in modes
    fail at the listed rank and stage and make the real run's collective calls after the failure."""
    r = subprocess.run([sys.executable, BENCH, "--gpus", str(world), "--check-launch", "--check-ladder", fails],
                       capture_output=True, text=True, timeout=600, env=_env())
    assert r.returncode == (0 if mode else 4), r.stderr[-3000:]
    line = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])
    assert line["ranks_seen"] == world
    d = line["exchange_decision"]
    assert d["mode"] == mode
    assert [a["mode"] for a in d["attempts"] if not a["ok"]] == failed
    for a in d["attempts"]:
        if not a["ok"]:   # the reason of every rank that failed, and only of those
            spec = [f for f in fails.split(",") if f.startswith(a["mode"] + ":")][0]
            who = spec.split("@")[1]
            assert set(a["why"]) == ({str(q) for q in range(world)} if who == "*" else {who}), a
            assert a["stage"] == spec.split(":")[1].split("@")[0]
