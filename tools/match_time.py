"""Time of bos_match_landmarks and bos_match_poses beside the route the library offered before them, on the
same handle (measurement, not a test):

    python3 tools/match_time.py          # c1, c2, c3
    python3 tools/match_time.py c2       # one step alone (c1 | c2 | c3)

Without an argument every step runs as a child process of its own under its own time limit, and the first
one that fails ends the run.

Per problem (fp64, default Schur plan, one handle, medians of 10 calls after one warm-up), k = 4, *_all off:
  landmarks  8 query landmarks (spread over the stix range), gate chi^2_2(0.99) = 9.21
  poses      8 relative-pose measurements taken from the last pose (the predictions toward eight earlier
             poses plus a small offset, Omega = diag(500, 500, 5000)), gate chi^2_3(0.99) = 11.34
  new   Solver.match_landmarks() / Solver.match_poses(): wall time and its split into host preparation (host
        clock), J+H build, factorization, selected inverse, column solve + gather, score kernel, selection
        (HIP events) and download (host clock);
  old   Solver.node_covariances(nodes, cross=False), then on the host the differences or errors, the 2 x 2 or
        3 x 3 solves, the gate and argpartition in NumPy: wall time, the node call's split and the host part.
Beside them the bytes each route downloads, the ratio of the wall times, and whether the two routes list
the same candidates."""
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "prb-project-bearing-only-slam_amd"))
import bos  # noqa: E402

LIMITS = {"c1": 180, "c2": 120, "c3": 420}
GATE_LM, GATE_POSE, K, N_QUERIES = 9.21, 11.34, 4, 8
OMEGA = np.diag([500.0, 500.0, 5000.0])


def problem(which):
    if which == "c1":
        return bos.load_g2o(os.path.join(ROOT, "tests", "golden", "data", "slam2D_bearing_only_initial_guess.g2o"))
    return bos.synthetic(1000, 2000, 20) if which == "c2" else bos.synthetic(100000, 200000, 10)


def predicted(pose_xyt, a):
    x, y, th = pose_xyt[a]
    dx, dy = pose_xyt[:, 0] - x, pose_xyt[:, 1] - y
    c, s = np.cos(th), np.sin(th)
    return np.stack([c * dx + s * dy, -s * dx + c * dy, (pose_xyt[:, 2] - th + np.pi) % (2 * np.pi) - np.pi], axis=1)


def timed(call, timing, n=10):
    call()
    wall, split = [], []
    for _ in range(n):
        t0 = time.perf_counter()
        call()
        wall.append(1e3 * (time.perf_counter() - t0))
        split.append(timing())
    return float(np.median(wall)), {k: float(np.median([d[k] for d in split])) for k in split[0]}


def quadratic(M, v):
    """v^T M^-1 v over stacks of symmetric 2 x 2 or 3 x 3 matrices; NaN where M is not positive definite."""
    with np.errstate(all="ignore"):
        ok = np.linalg.det(M) > 0
        y = np.linalg.solve(np.where(ok[..., None, None], M, np.eye(M.shape[-1])), v[..., None])[..., 0]
        return np.where(ok, (v * y).sum(axis=-1), np.nan)


def select(score, gate, kk):
    inside = np.isfinite(score) & (score <= gate)
    masked = np.where(inside, score, np.inf)
    part = np.argpartition(masked, kk - 1, axis=1)[:, :kk]
    order = np.take_along_axis(part, np.argsort(np.take_along_axis(masked, part, axis=1), axis=1), axis=1)
    return np.where(np.take_along_axis(inside, order, axis=1), order, -1), inside.sum(axis=1)


def report(which, what, S, new_call, old_call, host_ms, old, new_key, bytes_new, bytes_old, N):
    t0 = time.perf_counter()
    new = new_call()
    first = 1e3 * (time.perf_counter() - t0)
    w_new, t = timed(new_call, S.match_timing)
    print(f"{which} {what}: new route (solver_info {new['solver_info']}, first call {first:.1f} ms): wall {w_new:.3f} ms = prepare "
          f"{t['prepare_ms']:.3f} + J+H {t['jh_ms']:.3f} + factor {t['factor_ms']:.3f} + selected inverse {t['selinv_ms']:.3f} + column "
          f"solve+gather {t['column_ms']:.3f} + score kernel {t['score_ms']:.3f} + selection {t['select_ms']:.3f} + download "
          f"{t['download_ms']:.3f}; downloads {bytes_new} bytes; buffers {int(t['match_bytes'])} bytes", flush=True)
    w_old, tn = timed(old_call, S.node_covariances_timing)
    print(f"{which} {what}: old route: wall {w_old:.3f} ms = prepare {tn['prepare_ms']:.3f} + J+H {tn['jh_ms']:.3f} + factor {tn['factor_ms']:.3f} "
          f"+ selected inverse {tn['selinv_ms']:.3f} + column solve {tn['column_ms']:.3f} + gather+projection {tn['gather_ms']:.3f} "
          f"+ download {tn['download_ms']:.3f}, then NumPy scores + gate + argpartition {float(np.median(host_ms[1:])):.3f}; downloads "
          f"{bytes_old} bytes", flush=True)
    kk = min(K, N)
    same = np.array_equal(np.sort(old["cand"][:, :kk], axis=1), np.sort(new[new_key][:, :kk], axis=1))
    added = t["score_ms"] + t["select_ms"]
    print(f"{which} {what}: new / old wall {w_new / w_old:.2f} ({w_new:.3f} / {w_old:.3f} ms); downloaded bytes {bytes_new} / {bytes_old}; the "
          f"added launches {added:.3f} ms against the column solve+gather's {t['column_ms']:.3f}; counts inside the gate "
          f"{new['n_inside'].tolist()}; both routes list the same candidates: {same}", flush=True)


def measure(which):
    P = problem(which)
    S = bos.Solver(P, device=0)
    S.step()
    pose_xyt, lm_xy = S.get_state()
    print(f"{which}: NP {P.NP} NL {P.NL} n {S.system_info()['n']}; k {K}", flush=True)

    # landmarks: 8 queries, one column each on both routes
    lms = np.linspace(0, P.NL - 1, N_QUERIES).astype(np.int32)
    host_ms, old = [], {}

    def old_landmarks():
        C = S.node_covariances(P.NP + lms, cross=False)["projected_landmark"]
        t1 = time.perf_counter()
        d = lm_xy[lms][:, None, :] - lm_xy[None, :, :]
        d2 = quadratic(C.reshape(len(lms), P.NL, 2, 2), d)
        d2[np.arange(len(lms)), lms] = np.nan
        old["cand"], old["count"] = select(d2, GATE_LM, min(K, P.NL))
        host_ms.append(1e3 * (time.perf_counter() - t1))

    report(which, f"landmarks ({N_QUERIES} queries, gate {GATE_LM})", S, lambda: S.match_landmarks(lms, gate=GATE_LM, k=K), old_landmarks,
           host_ms, old, "cand_landmark", N_QUERIES * (K * (4 + 8 * (1 + 2 + 4)) + 4), 8 * N_QUERIES * (9 * P.NP + 4 * P.NL), P.NL)

    # poses: 8 measurements from the last pose, one column on both routes
    a = P.NP - 1 if P.fixed != P.NP - 1 else P.NP - 2
    pred = predicted(pose_xyt, a)
    targets = (a - 5 - 7 * np.arange(N_QUERIES)) % P.NP
    z = pred[targets] + np.array([0.02, -0.01, 0.004])
    pose = np.full(N_QUERIES, a, dtype=np.int32)
    R = np.linalg.inv(OMEGA)
    host_ms2, old2 = [], {}

    def old_poses():
        Pm = S.node_covariances([a], cross=False)["projected_pose"][0]
        t1 = time.perf_counter()
        e = predicted(pose_xyt, a)[None, :, :] - z[:, None, :]
        e[:, :, 2] = (e[:, :, 2] + np.pi) % (2 * np.pi) - np.pi
        nis = quadratic(np.broadcast_to(Pm.reshape(P.NP, 3, 3) + R, (len(z), P.NP, 3, 3)), e)
        old2["cand"], old2["count"] = select(nis, GATE_POSE, min(K, P.NP))
        host_ms2.append(1e3 * (time.perf_counter() - t1))

    report(which, f"poses ({N_QUERIES} measurements from pose {a}, gate {GATE_POSE})", S,
           lambda: S.match_poses(pose, z, OMEGA, gate=GATE_POSE, k=K), old_poses, host_ms2, old2, "cand_pose",
           N_QUERIES * (K * (4 + 8 * (1 + 3 + 9)) + 4), 8 * (9 * P.NP + 4 * P.NL), P.NP)
    S.close()


if __name__ == "__main__":
    if len(sys.argv) > 1:
        measure(sys.argv[1])
        sys.exit(0)
    for step in ("c1", "c2", "c3"):
        rc = subprocess.call(["timeout", "-k", "10", str(LIMITS[step]), sys.executable, os.path.abspath(__file__), step])
        if rc != 0:
            print(f"{step}: exit status {rc}; stopping", flush=True)
            sys.exit(rc)
