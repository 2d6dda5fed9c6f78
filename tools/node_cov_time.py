"""Time of bos_node_covariances beside bos_pair_covariances asked for the same column, on the same handle
(measurement, not a test):

    python3 tools/node_cov_time.py                     # c1, c2, c3
    python3 tools/node_cov_time.py c2                  # one step alone (c1 | c2 | c3)
    python3 tools/node_cov_time.py base c2 [--lib F]   # step(), marginals() and pair_covariances() alone,
                                                       # optionally with another build of libbos.so
    python3 tools/node_cov_time.py ab F                # five interleaved passes of base (F, this tree, F, ...)
                                                       # on c1, c2, c3 and the ranges of each figure

Without an argument every step runs as a child process of its own under its own time limit, and
the first one that fails ends the run.

Per problem (fp64, default Schur plan, medians of 10 calls after one warm-up), for 1 and 8 query nodes
(the last pose; then seven seeded random nodes, poses and landmarks) with all four node outputs and with
the cross blocks alone: the wall time of Solver.node_covariances() and its split into host preparation
(host clock), J+H build, factorization, selected inverse, column solve, gather + projection (HIP events)
and download (host clock). Beside them, on the same handle: pair_covariances() asked for the last pose's
column (the pairs (a, u) for every node u), with all outputs and with the cross blocks alone."""
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "prb-project-bearing-only-slam_amd"))
import bos  # noqa: E402

LIMITS = {"c1": 180, "c2": 120, "c3": 420}
NAMES = {"c1": "C1      ", "c2": "config 2", "c3": "config 3"}
PASSES = 5


def problem(which):
    if which == "c1":
        return bos.load_g2o(os.path.join(ROOT, "tests", "golden", "data", "slam2D_bearing_only_initial_guess.g2o"))
    return bos.synthetic(1000, 2000, 20) if which == "c2" else bos.synthetic(100000, 200000, 10)


def query_nodes(P, n, seed=31):
    """The last free pose, then n - 1 seeded random nodes."""
    last = P.NP - 1 if P.fixed != P.NP - 1 else P.NP - 2
    rest = np.random.default_rng(seed).integers(0, P.NP + P.NL, max(n - 1, 0))
    return np.concatenate([[last], rest]).astype(np.int32)


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
    column = {}
    for count in (1, 8):
        nodes = query_nodes(P, count)
        for projected in (True, False):
            t0 = time.perf_counter()
            info = S.node_covariances(nodes, projected=projected)["solver_info"]
            first = 1e3 * (time.perf_counter() - t0)
            w, t = timed(lambda: S.node_covariances(nodes, projected=projected), S.node_covariances_timing)
            column[(count, projected)] = (w, t)
            print(f"{which}: {count} nodes, {'cross + projected' if projected else 'cross alone'} (solver_info {info}, first call "
                  f"{first:.1f} ms): wall {w:.3f} ms = prepare {t['prepare_ms']:.3f} + J+H {t['jh_ms']:.3f} + factor {t['factor_ms']:.3f} "
                  f"+ selected inverse {t['selinv_ms']:.3f} + column solve {t['column_ms']:.3f} + gather+projection {t['gather_ms']:.3f} "
                  f"+ download {t['download_ms']:.3f}; buffers {int(t['node_bytes'])} bytes", flush=True)
    a = int(query_nodes(P, 1)[0])
    pa = np.full(P.NP + P.NL, a, dtype=np.int32)
    pb = np.arange(P.NP + P.NL, dtype=np.int32)
    for projected in (True, False):
        kw = dict(projected=projected, blocks=projected)
        w, t = timed(lambda: S.pair_covariances(pa, pb, **kw), S.pair_covariances_timing)
        wc, tc = column[(1, projected)]
        own_p = t["prepare_ms"] + t["path_ms"] + t["product_ms"] + t["download_ms"]
        own_c = tc["prepare_ms"] + tc["selinv_ms"] + tc["column_ms"] + tc["gather_ms"] + tc["download_ms"]
        print(f"{which}: same handle, pair_covariances for the column of node {a} ({len(pa)} pairs), "
              f"{'all outputs' if projected else 'cross alone'}: wall {w:.3f} ms = prepare+upload {t['prepare_ms']:.3f} + J+H {t['jh_ms']:.3f} "
              f"+ factor {t['factor_ms']:.3f} + path solve {t['path_ms']:.3f} + product+projection {t['product_ms']:.3f} + download "
              f"{t['download_ms']:.3f}; column call / pair route: wall {wc / w:.2f}, past the factorization {own_c / own_p:.2f} "
              f"({own_c:.3f} / {own_p:.3f} ms); the column call's download is {100 * tc['download_ms'] / wc:.0f} % of its wall time",
              flush=True)
    S.close()


def base(which, lib):
    """step(), marginals() and pair_covariances() (1 000 seeded pairs) alone: wall ms, medians of 10 after a warm-up."""
    if lib:
        bos.LIB_PATH = os.path.abspath(lib)
        bos.ALLOW_MISSING_SYMBOLS = True
    P = problem(which)
    S = bos.Solver(P, device=0)
    S.step()
    rng = np.random.default_rng(29)
    a, b = rng.integers(0, P.NP, 1000).astype(np.int32), (P.NP + rng.integers(0, P.NL, 1000)).astype(np.int32)
    w_m, m = timed(S.marginals, S.marginals_timing)
    w_p, _ = timed(lambda: S.pair_covariances(a, b), S.pair_covariances_timing)
    S.step()
    steps = []
    for _ in range(10):
        t0 = time.perf_counter()
        st = S.step()
        steps.append((1e3 * (time.perf_counter() - t0), st["t_solve_ms"]))
    w_s, t_s = (float(np.median([x[i] for x in steps])) for i in (0, 1))
    print(f"{which} {'other' if lib else 'this '}: marginals {w_m:.3f} (sel. inv. {m['selinv_ms']:.3f})  pair_covariances {w_p:.3f}  "
          f"step {w_s:.3f} (solve {t_s:.3f})", flush=True)
    S.close()
    return {"marginals": w_m, "pair_covariances": w_p, "step": w_s, "step t_solve_ms": t_s}


def ab(lib):
    """PASSES interleaved passes of base, each a process of its own per problem, then every figure's range."""
    import re
    seen = {}
    for _ in range(PASSES):
        for which in ("c1", "c2", "c3"):
            for other in (True, False):
                cmd = ["timeout", "-k", "10", str(LIMITS[which]), sys.executable, os.path.abspath(__file__), "base", which]
                r = subprocess.run(cmd + (["--lib", lib] if other else []), capture_output=True, text=True)
                sys.stdout.write(r.stdout)
                sys.stdout.flush()
                if r.returncode != 0:
                    print(f"{which}: exit status {r.returncode}; stopping\n{r.stderr[-2000:]}", flush=True)
                    sys.exit(r.returncode)
                line = r.stdout.strip().splitlines()[-1]
                v = [float(x) for x in re.findall(r"(\d+\.\d+)", line)]
                for key, x in zip(("marginals", "sel", "pair_covariances", "step", "step t_solve_ms"), v):
                    seen.setdefault((which, key, other), []).append(x)
    print()
    worst = 0.0
    for which in ("c1", "c2", "c3"):
        for key in ("marginals", "pair_covariances", "step", "step t_solve_ms"):
            o, t = seen[(which, key, True)], seen[(which, key, False)]
            worst = max(worst, max(t) - max(o))
            print(f"  {NAMES[which]} {key:16s} parent {min(o):7.3f} .. {max(o):7.3f} (median {np.median(o):7.3f}), this tree "
                  f"{min(t):7.3f} .. {max(t):7.3f} (median {np.median(t):7.3f})")
    print(f"Largest excess of this tree's slowest pass over the parent's slowest pass: {worst:.3f} ms")


if __name__ == "__main__":
    if len(sys.argv) > 2 and sys.argv[1] == "ab":
        ab(os.path.abspath(sys.argv[2]))
        sys.exit(0)
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
