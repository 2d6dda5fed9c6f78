"""Time of bos_joint_compatibility beside the route the library offered before it, on the same handle
(measurement, not a test):

    python3 tools/joint_time.py [--out FILE]           # c1, c2, c3; FILE defaults to profiles/r15_joint.txt
    python3 tools/joint_time.py c2                     # one step alone (c1 | c2 | c3), to stdout
    python3 tools/joint_time.py ab OTHER_LIBBOS [--passes N] [c1 c2 c3]   # step() and pair_covariances() on this build and another

Without an argument every step runs as a child process of its own under its own time limit, and the first
one that fails ends the run.

Per problem (fp64, default Schur plan, one handle, medians of 10 calls after one warm-up), two workloads:
  branches  256 hypotheses of 8 pairings: 8 bearings taken from one pose, each assigned to one of 16 candidate
            landmarks (seeded), omega = 400
  one32     one hypothesis of 32 pairings over 32 seeded poses, each with a landmark it observes
  new   Solver.joint_compatibility(): wall time and its split into host preparation + upload (host clock), J+H
        build, factorization, path solve, products, NIS kernel (HIP events) and download (host clock);
  old   Solver.pair_covariances() over all distinct node pairs of the hypotheses (cross and blocks), then on the
        host the assembly of Sigma over the call's nodes, S = J Sigma J^T + R per hypothesis and
        numpy.linalg.solve: wall time, the pair call's split and the host part.
Beside them the bytes each route downloads, the ratio of the wall times and the largest relative difference of
the two routes' joint NIS.

ab: PASSES (or N) interleaved passes, each a process of its own per problem and build: step() and pair_covariances()
(1 000 seeded pairs), wall ms, medians of 10 after a warm-up; then every figure's range per build."""
import os
import re
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "prb-project-bearing-only-slam_amd"))
import bos  # noqa: E402

LIMITS = {"c1": 180, "c2": 120, "c3": 420}
PASSES = 3
OMEGA = 400.0


def problem(which):
    if which == "c1":
        return bos.load_g2o(os.path.join(ROOT, "tests", "golden", "data", "slam2D_bearing_only_initial_guess.g2o"))
    return bos.synthetic(1000, 2000, 20) if which == "c2" else bos.synthetic(100000, 200000, 10)


def timed(call, timing, n=10):
    call()
    wall, split = [], []
    for _ in range(n):
        t0 = time.perf_counter()
        call()
        wall.append(1e3 * (time.perf_counter() - t0))
        split.append(timing())
    return float(np.median(wall)), {k: float(np.median([d[k] for d in split])) for k in split[0]}


def bearing(pose_xyt, lm_xy, p, l):
    x, y, th = pose_xyt[p].T
    dx, dy = lm_xy[l, 0] - x, lm_xy[l, 1] - y
    c, s = np.cos(th), np.sin(th)
    return np.arctan2(-s * dx + c * dy, c * dx + s * dy)


def jacobians(pose, lm):
    """[M, 5]: the bearing Jacobian over [pose dofs | landmark dofs] (csrc/host/bos_math.hpp bearing_error_jacobian)."""
    c, s = np.cos(pose[:, 2]), np.sin(pose[:, 2])
    dx, dy = lm[:, 0] - pose[:, 0], lm[:, 1] - pose[:, 1]
    gx, gy = c * dx + s * dy, -s * dx + c * dy
    f = 1.0 / (gx * gx + gy * gy)
    a0, a1 = -f * gy, f * gx
    J = np.zeros((len(pose), 5))
    J[:, 3], J[:, 4] = a0 * c - a1 * s, a0 * s + a1 * c
    J[:, 0], J[:, 1] = -J[:, 3], -J[:, 4]
    J[:, 2] = a0 * (c * lm[:, 1] - s * lm[:, 0]) + a1 * (-s * lm[:, 1] - c * lm[:, 0])
    return J


def old_route(P, S, state, start, pose, lm, z, omega, host_ms):
    """joint NIS per hypothesis through pair_covariances() and NumPy."""
    pose_xyt, lm_xy = state
    nodes = np.unique(np.concatenate([pose, P.NP + lm]))
    ia, ib = np.triu_indices(len(nodes), 1)
    out = S.pair_covariances(np.concatenate([nodes[ia], nodes]), np.concatenate([nodes[ib], nodes]), projected=False)
    t1 = time.perf_counter()
    d = np.where(nodes < P.NP, 3, 2)
    off = np.concatenate([[0], np.cumsum(d)])
    Sig = np.zeros((off[-1], off[-1]))
    for q, (a, b) in enumerate(zip(ia, ib)):
        blk = out["cross"][q, :d[a] * d[b]].reshape(d[a], d[b])
        Sig[off[a]:off[a + 1], off[b]:off[b + 1]] = blk
        Sig[off[b]:off[b + 1], off[a]:off[a + 1]] = blk.T
    for a in range(len(nodes)):
        Sig[off[a]:off[a + 1], off[a]:off[a + 1]] = out["cov_a"][len(ia) + a, :d[a] * d[a]].reshape(d[a], d[a])
    slot = {int(u): i for i, u in enumerate(nodes)}
    J = jacobians(pose_xyt[pose], lm_xy[lm])
    e = (bearing(pose_xyt, lm_xy, pose, lm) - z + np.pi) % (2 * np.pi) - np.pi
    nis = np.zeros(len(start) - 1)
    for h in range(len(start) - 1):
        q = np.arange(start[h], start[h + 1])
        dofs = np.array([list(range(off[slot[int(pose[i])]], off[slot[int(pose[i])]] + 3)) +
                         list(range(off[slot[int(P.NP + lm[i])]], off[slot[int(P.NP + lm[i])]] + 2)) for i in q])      # [m, 5]
        blk = Sig[np.ix_(dofs.ravel(), dofs.ravel())].reshape(len(q), 5, len(q), 5)
        Sh = np.einsum("ia,iajb,jb->ij", J[q], blk, J[q]) + np.diag(1.0 / omega[q])
        nis[h] = e[q] @ np.linalg.solve(Sh, e[q])
    host_ms.append(1e3 * (time.perf_counter() - t1))
    return nis, 9 * 8 * 3 * len(out["cross"])


def report(say, which, what, P, S, state, start, pose, lm, z, omega):
    new_call = lambda: S.joint_compatibility((start, pose, lm), z, omega)
    t0 = time.perf_counter()
    new = new_call()
    first = 1e3 * (time.perf_counter() - t0)
    w_new, t = timed(new_call, S.joint_compatibility_timing)
    bytes_new = 8 * (2 * len(pose) + len(start) - 1)
    say(f"{which} {what}: new route (solver_info {new['solver_info']}, first call {first:.1f} ms): wall {w_new:.3f} ms = prepare+upload "
        f"{t['prepare_ms']:.3f} + J+H {t['jh_ms']:.3f} + factor {t['factor_ms']:.3f} + path solve {t['path_ms']:.3f} + products "
        f"{t['product_ms']:.3f} + NIS kernel {t['nis_ms']:.3f} + download {t['download_ms']:.3f}; downloads {bytes_new} bytes; buffers "
        f"{int(t['joint_bytes'])} bytes")
    host_ms, res = [], {}

    def old_call():
        res["nis"], res["bytes"] = old_route(P, S, state, start, pose, lm, z, omega, host_ms)

    w_old, tp = timed(old_call, S.pair_covariances_timing)
    say(f"{which} {what}: old route: wall {w_old:.3f} ms = prepare+upload {tp['prepare_ms']:.3f} + J+H {tp['jh_ms']:.3f} + factor "
        f"{tp['factor_ms']:.3f} + path solve {tp['path_ms']:.3f} + products+projection {tp['product_ms']:.3f} + download "
        f"{tp['download_ms']:.3f}, then NumPy assembly + solves {float(np.median(host_ms[1:])):.3f}; downloads {res['bytes']} bytes")
    rel = float(np.max(np.abs(res["nis"] - new["joint_nis"]) / np.maximum(np.abs(new["joint_nis"]), 1e-300)))
    say(f"{which} {what}: new / old wall {w_new / w_old:.3f} ({w_new:.3f} / {w_old:.3f} ms), old / new {w_old / w_new:.2f}; past the "
        f"factorization {t['prepare_ms'] + t['path_ms'] + t['product_ms'] + t['nis_ms'] + t['download_ms']:.3f} ms against "
        f"{w_old - tp['jh_ms'] - tp['factor_ms']:.3f}; downloaded bytes {bytes_new} / {res['bytes']}; largest relative difference of the "
        f"joint NIS {rel:.3g}")


def measure(which, say):
    P = problem(which)
    S = bos.Solver(P, device=0)
    S.step()
    state = S.get_state()
    pose_xyt, lm_xy = state
    rng = np.random.default_rng(41)
    say(f"{which}: NP {P.NP} NL {P.NL} n {S.system_info()['n']}")
    free = np.array([p for p in range(max(0, P.NP - 4000), P.NP) if p != P.fixed])
    a = int(free[-1])
    seen = np.unique(P.b_lm[P.b_pose == a])
    cand = np.unique(np.concatenate([seen, (int(seen[0]) if len(seen) else 0) + np.arange(32)]) % P.NL)[:16]
    truth = rng.choice(cand, 8, replace=False)
    zb = bearing(pose_xyt, lm_xy, np.full(8, a), truth) + 0.02 * rng.standard_normal(8)
    n_hyp = 256
    start = 8 * np.arange(n_hyp + 1, dtype=np.int32)
    pose = np.full(8 * n_hyp, a, dtype=np.int32)
    lm = rng.choice(cand, (n_hyp, 8)).astype(np.int32)
    lm[0] = truth
    report(say, which, f"branches (256 x 8 from pose {a}, 16 candidates)", P, S, state, start, pose, lm.ravel(), np.tile(zb, n_hyp),
           np.full(8 * n_hyp, OMEGA))
    observing = np.unique(P.b_pose[np.isin(P.b_pose, free)])
    poses = rng.choice(observing, 32, replace=False).astype(np.int32)
    lms = np.array([P.b_lm[P.b_pose == p][0] for p in poses], dtype=np.int32)
    z1 = bearing(pose_xyt, lm_xy, poses, lms) + 0.02 * rng.standard_normal(32)
    report(say, which, "one32 (1 x 32 over 32 poses)", P, S, state, np.array([0, 32], dtype=np.int32), poses, lms, z1, np.full(32, OMEGA))
    S.close()


def base(which, lib):
    """step() and pair_covariances() (1 000 seeded pairs) alone: wall ms, medians of 10 after a warm-up."""
    if lib:
        bos.LIB_PATH = os.path.abspath(lib)
        bos.ALLOW_MISSING_SYMBOLS = True
    P = problem(which)
    S = bos.Solver(P, device=0)
    S.step()
    rng = np.random.default_rng(29)
    a, b = rng.integers(0, P.NP, 1000).astype(np.int32), (P.NP + rng.integers(0, P.NL, 1000)).astype(np.int32)
    w_p, _ = timed(lambda: S.pair_covariances(a, b), S.pair_covariances_timing)
    S.step()
    steps = []
    for _ in range(10):
        t0 = time.perf_counter()
        S.step()
        steps.append(1e3 * (time.perf_counter() - t0))
    print(f"{which} {'other' if lib else 'this '}: pair_covariances {w_p:.3f}  step {float(np.median(steps)):.3f}", flush=True)
    S.close()


def ab(lib, problems, passes):
    seen = {}
    for i in range(passes):
        for which in problems:
            for other in ((True, False) if i % 2 == 0 else (False, True)):   # the build that goes first alternates
                cmd = ["timeout", "-k", "10", str(LIMITS[which]), sys.executable, os.path.abspath(__file__), "base", which]
                r = subprocess.run(cmd + (["--lib", lib] if other else []), capture_output=True, text=True)
                sys.stdout.write(r.stdout)
                sys.stdout.flush()
                if r.returncode != 0:
                    print(f"{which}: exit status {r.returncode}; stopping\n{r.stderr[-2000:]}", flush=True)
                    sys.exit(r.returncode)
                v = [float(x) for x in re.findall(r"(\d+\.\d+)", r.stdout.strip().splitlines()[-1])]
                for key, x in zip(("pair_covariances", "step"), v):
                    seen.setdefault((which, key, other), []).append(x)
    print()
    for (which, key, other), v in sorted(seen.items()):
        print(f"{which} {key:17s} {'other' if other else 'this '}: min {min(v):.3f} median {float(np.median(v)):.3f} max {max(v):.3f} ms "
              f"over {len(v)} interleaved passes", flush=True)


if __name__ == "__main__":
    args = sys.argv[1:]
    if args and args[0] in LIMITS:
        measure(args[0], lambda s: print(s, flush=True))
        sys.exit(0)
    if args and args[0] == "base":
        base(args[1], args[3] if len(args) > 3 and args[2] == "--lib" else None)
        sys.exit(0)
    if args and args[0] == "ab":
        rest = args[2:]
        passes = PASSES
        if rest[:1] == ["--passes"]:
            passes, rest = int(rest[1]), rest[2:]
        ab(args[1], rest or ["c1", "c2", "c3"], passes)
        sys.exit(0)
    out = args[1] if len(args) > 1 and args[0] == "--out" else os.path.join(ROOT, "profiles", "r15_joint.txt")
    with open(out, "w") as f:
        for step in ("c1", "c2", "c3"):
            r = subprocess.run(["timeout", "-k", "10", str(LIMITS[step]), sys.executable, os.path.abspath(__file__), step],
                               stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
            sys.stdout.write(r.stdout)
            sys.stdout.flush()
            f.write(r.stdout)
            f.flush()
            if r.returncode != 0:
                print(f"{step}: exit status {r.returncode}; stopping\n{r.stderr[-2000:]}", flush=True)
                sys.exit(r.returncode)
