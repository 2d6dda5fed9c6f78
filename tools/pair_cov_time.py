"""Time of bos_pair_covariances beside bos_edge_covariances and a GN step on the same handle
(measurement, not a test):

    python3 tools/pair_cov_time.py                     # c1, c2, c3
    python3 tools/pair_cov_time.py c2                  # one step alone (c1 | c2 | c3)
    python3 tools/pair_cov_time.py base c2 [--lib F]   # marginals(), edge_covariances() and step() alone,
                                                       # optionally with another build of libbos.so (A/B
                                                       # passes against the parent commit)

Without an argument every step runs as a child process of its own under its own time limit, and
the first one that fails ends the run.

Per problem (fp64, default Schur plan, medians of 10 calls after one warm-up) and for 1, 1 000 and
100 000 seeded random pairs (a third of each kind): the wall time of Solver.pair_covariances() with all
outputs, its split into host preparation and upload (host clock), J+H build, factorization, path solve,
product and projection (HIP events) and download (host clock), the distinct nodes of the call, and the
bytes of the feature's buffers. Beside them, on the same handle: the device time of edge_covariances()
(the only other source of a cross block) and a step's t_solve_ms."""
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "prb-project-bearing-only-slam_amd"))
import bos  # noqa: E402

LIMITS = {"c1": 180, "c2": 120, "c3": 420}
SIZES = (1, 1000, 100000)


def problem(which):
    if which == "c1":
        return bos.load_g2o(os.path.join(ROOT, "tests", "golden", "data", "slam2D_bearing_only_initial_guess.g2o"))
    return bos.synthetic(1000, 2000, 20) if which == "c2" else bos.synthetic(100000, 200000, 10)


def pairs(P, n, seed=29):
    """n seeded random pairs, a third of each kind (pose-pose, pose-landmark, landmark-landmark)."""
    rng = np.random.default_rng(seed)
    kind = np.arange(n) % 3
    a = np.where(kind < 2, rng.integers(0, P.NP, n), P.NP + rng.integers(0, P.NL, n))
    b = np.where(kind < 1, rng.integers(0, P.NP, n), P.NP + rng.integers(0, P.NL, n))
    return a.astype(np.int32), b.astype(np.int32)


def timed(call, timing, n=10):
    call()
    wall, split = [], []
    for _ in range(n):
        t0 = time.perf_counter()
        call()
        wall.append(1e3 * (time.perf_counter() - t0))
        split.append(timing())
    return float(np.median(wall)), {k: float(np.median([d[k] for d in split])) for k in split[0]}


def measure(which):
    P = problem(which)
    S = bos.Solver(P, device=0)
    S.step()
    n = S.system_info()["n"]
    print(f"{which}: NP {P.NP} NL {P.NL} Mb {len(P.b_z)} Mo {len(P.o_z)} n {n}")
    for count in SIZES:
        a, b = pairs(P, count)
        t0 = time.perf_counter()
        info = S.pair_covariances(a, b)["solver_info"]
        first = 1e3 * (time.perf_counter() - t0)
        w, t = timed(lambda: S.pair_covariances(a, b), S.pair_covariances_timing)
        distinct = len(np.setdiff1d(np.unique(np.concatenate([a, b])), [P.fixed]))
        dev = t["jh_ms"] + t["factor_ms"] + t["path_ms"] + t["product_ms"]
        print(f"{which}: {count} pairs ({distinct} distinct nodes, solver_info {info}, first call {first:.1f} ms): wall {w:.3f} ms = "
              f"prepare+upload {t['prepare_ms']:.3f} + J+H {t['jh_ms']:.3f} + factor {t['factor_ms']:.3f} + path solve {t['path_ms']:.3f} "
              f"+ product+projection {t['product_ms']:.3f} + download {t['download_ms']:.3f}; device {dev:.3f} ms; "
              f"buffers {int(t['pair_bytes'])} bytes", flush=True)
    _, e = timed(S.edge_covariances, S.edge_covariances_timing)
    dev_e = e["jh_ms"] + e["factor_ms"] + e["selinv_ms"] + e["project_ms"]
    solve = float(np.median([S.step()["t_solve_ms"] for _ in range(10)]))
    print(f"{which}: same handle: edge_covariances device {dev_e:.3f} ms (factor {e['factor_ms']:.3f}, selected inverse "
          f"{e['selinv_ms']:.3f}); step t_solve_ms {solve:.3f}", flush=True)
    S.close()


def base(which, lib):
    """marginals(), edge_covariances() and step() alone: wall ms, medians of 10 after a warm-up."""
    if lib:
        bos.LIB_PATH = os.path.abspath(lib)
        bos.ALLOW_MISSING_SYMBOLS = True
    P = problem(which)
    S = bos.Solver(P, device=0)
    S.step()
    w_m, m = timed(S.marginals, S.marginals_timing)
    w_e, e = timed(S.edge_covariances, S.edge_covariances_timing)
    S.step()
    steps = []
    for _ in range(10):
        t0 = time.perf_counter()
        st = S.step()
        steps.append((1e3 * (time.perf_counter() - t0), st["t_solve_ms"]))
    w_s, t_s = (float(np.median([x[i] for x in steps])) for i in (0, 1))
    print(f"{which} {'other' if lib else 'this '}: marginals {w_m:.3f} (sel. inv. {m['selinv_ms']:.3f})  edge_covariances {w_e:.3f} "
          f"(sel. inv. {e['selinv_ms']:.3f})  step {w_s:.3f} (solve {t_s:.3f})", flush=True)
    S.close()


if __name__ == "__main__":
    if len(sys.argv) > 2 and sys.argv[1] == "base":
        base(sys.argv[2], sys.argv[4] if len(sys.argv) > 4 and sys.argv[3] == "--lib" else None)
        sys.exit(0)
    if len(sys.argv) > 1:
        measure(sys.argv[1])
        sys.exit(0)
    for step in ("c1", "c2", "c3"):
        rc = subprocess.call(["timeout", "-k", "10", str(LIMITS[step]), sys.executable, os.path.abspath(__file__), step])
        if rc != 0:
            print(f"{step}: exit status {rc}; stopping", flush=True)
            sys.exit(rc)
