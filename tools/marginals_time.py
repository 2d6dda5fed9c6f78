"""Time of bos_marginals beside the solve of a GN step (measurement, not a test):

    python3 tools/marginals_time.py            # c1, c2, c3, then the config-3 spot check
    python3 tools/marginals_time.py c2         # one step alone (c1 | c2 | c3 | spot3)

Without an argument every step runs as a child process of its own under its own time limit, and
the first one that fails ends the run (the shell form of the same thing:
    timeout -k 10 120 python3 tools/marginals_time.py c1 && timeout -k 10 120 python3 tools/marginals_time.py c2 && ...).

Per problem: the wall time of Solver.marginals() (median of 10 calls after one warm-up), its split
into J+H build, factorization, selected inverse (HIP events) and download (host clock), the bytes
of the Sigma-front buffer, and t_solve_ms of a bos_step on the same handle (factorization + both
substitutions on the same tree: the yardstick). spot3: at config 3 no dense reference exists; 8
seeded random nodes are checked by solving H X = E for their unit columns (SuperLU on the exported
system) and the correlation-scaled error of their blocks is printed (no derived bound: kappa is
unknown at that size)."""
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "prb-project-bearing-only-slam_amd"))
import bos  # noqa: E402

LIMITS = {"c1": 120, "c2": 120, "c3": 300, "spot3": 900}


def problem(which):
    if which == "c1":
        return bos.load_g2o(os.path.join(ROOT, "tests", "golden", "data", "slam2D_bearing_only_initial_guess.g2o"))
    return bos.synthetic(1000, 2000, 20) if which == "c2" else bos.synthetic(100000, 200000, 10)


def measure(which):
    P = problem(which)
    S = bos.Solver(P, device=0)
    S.step()
    solve = float(np.median([S.step()["t_solve_ms"] for _ in range(10)]))
    S.marginals()
    wall, split = [], []
    for _ in range(10):
        t0 = time.perf_counter()
        _, _, info = S.marginals()
        wall.append(1e3 * (time.perf_counter() - t0))
        split.append(S.marginals_timing())
    med = lambda k: float(np.median([d[k] for d in split]))
    sel = med("selinv_ms")
    print(f"{which}: NP {P.NP} NL {P.NL} n {S.system_info()['n']} solver_info {info}")
    print(f"{which}: marginals wall {np.median(wall):.3f} ms = J+H {med('jh_ms'):.3f} + factor {med('factor_ms'):.3f} "
          f"+ selected inverse {sel:.3f} + download {med('download_ms'):.3f} (+ host)")
    print(f"{which}: step t_solve_ms {solve:.3f}; selected inverse / t_solve {sel / solve:.2f}, "
          f"marginals / t_solve {np.median(wall) / solve:.2f}")
    print(f"{which}: Sigma-front buffer {split[-1]['sigma_bytes']} bytes ({split[-1]['sigma_bytes'] / 2**20:.1f} MiB)", flush=True)
    S.close()


def spot3():
    import scipy.sparse as sp
    import scipy.sparse.linalg as spla
    P = problem("c3")
    S = bos.Solver(P, device=0)
    pose, lm, info = S.marginals()
    rows, cols, vals, _ = S.export_system()
    S.close()
    Hl = sp.coo_matrix((vals, (rows.astype(np.int64), cols.astype(np.int64))), shape=(P.N, P.N)).tocsr()
    keep = np.ones(P.N, dtype=bool)
    keep[3 * P.fixed:3 * P.fixed + 3] = False
    idx = np.nonzero(keep)[0]
    pos = -np.ones(P.N, dtype=np.int64)
    pos[idx] = np.arange(len(idx))
    H = (Hl + sp.tril(Hl, -1).T).tocsc()[idx][:, idx].tocsc()
    lu = spla.splu(H, permc_spec="MMD_AT_PLUS_A", diag_pivot_thresh=0.0, options=dict(SymmetricMode=True))
    rng = np.random.default_rng(7)
    nodes = [u for u in rng.choice(P.NP + P.NL, size=12, replace=False) if u != P.fixed][:8]
    worst = 0.0
    for u in nodes:
        d0, sz = (3 * u, 3) if u < P.NP else (3 * P.NP + 2 * (u - P.NP), 2)
        E = np.zeros((len(idx), sz))
        E[pos[d0:d0 + sz], np.arange(sz)] = 1.0
        ref = lu.solve(E)[pos[d0:d0 + sz]]
        out = pose[u] if u < P.NP else lm[u - P.NP]
        s = np.sqrt(np.diag(ref))
        e = float((np.abs(out - ref) / np.outer(s, s)).max())
        worst = max(worst, e)
        print(f"spot3: node {u} ({'pose' if u < P.NP else 'landmark'}) scaled error {e:.3g}")
    print(f"spot3: solver_info {info}, worst scaled error over {len(nodes)} nodes {worst:.3g}", flush=True)


if __name__ == "__main__":
    if len(sys.argv) > 1:
        spot3() if sys.argv[1] == "spot3" else measure(sys.argv[1])
        sys.exit(0)
    for step in ("c1", "c2", "c3", "spot3"):
        rc = subprocess.call(["timeout", "-k", "10", str(LIMITS[step]), sys.executable, os.path.abspath(__file__), step])
        if rc != 0:
            print(f"{step}: exit status {rc}; stopping", flush=True)
            sys.exit(rc)
