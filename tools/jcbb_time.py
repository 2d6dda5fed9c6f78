"""Time of bos_jcbb beside the routes the library offered before it, on the same handle (measurement, not a
test):

    python3 tools/jcbb_time.py [--out FILE]           # c1, c2, c3; FILE defaults to profiles/r16_jcbb.txt
    python3 tools/jcbb_time.py c2                     # one step alone (c1 | c2 | c3), to stdout
    python3 tools/jcbb_time.py ab OTHER_LIBBOS [--passes N] [c1 c2 c3]   # step() and joint_compatibility() on this build and another

Without an argument every step runs as a child process of its own under its own time limit, and the first one
that fails ends the run.

Per problem (fp64, default Schur plan, one handle, medians of 10 calls after one warm-up), three workloads whose
candidate lists come from associate_bearings() at the gate of one degree of freedom (omega = 400, z = the
predicted bearing of a landmark the pose observes + 0.02 N(0, 1)):
  one8x4    one frame of 8 bearings x up to 4 candidates from one pose
  one16x2   one frame of 16 bearings x up to 2 candidates
  many8x4   64 frames of 8 x 4 from 64 poses
  new   Solver.jcbb(): wall time, its split into host preparation + upload (host clock), J+H build, factorization,
        path solve, products, assembly + search kernel (HIP events) and download (host clock), and the nodes visited;
  old a Solver.joint_compatibility(all pairings, cov=True), then bos.jcbb_search_host per frame: the compiled serial
        search on the downloaded S (the fair baseline);
  old b the same call, then a NumPy depth-first search with the same prunings (numpy.linalg.solve per node); medians
        of 3 calls for one frame, one call after the warm-up for 64 frames.
Beside them the ratio of the wall times and whether the three routes return the same assignment.

ab: PASSES (or N) interleaved passes, each a process of its own per problem and build: step() and
joint_compatibility() (256 hypotheses of 8), wall ms, medians of 10 after a warm-up; then every figure's range per build."""
import os
import re
import subprocess
import sys
import time

import numpy as np
from scipy.stats import chi2

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from joint_time import LIMITS, ROOT, bearing, problem, timed  # noqa: E402

import bos  # noqa: E402

PASSES = 3
OMEGA = 400.0
GATES = chi2.ppf(0.95, np.arange(1, bos.JOINT_MAX_M + 1))


def numpy_search(cands, S, e, gate):
    """Depth first with the gate cut and the count bound; the NIS of a node by numpy.linalg.solve."""
    m = len(cands)
    start = np.concatenate([[0], np.cumsum([len(c) for c in cands])]).astype(int)
    rem = [sum(1 for c in cands[b + 1:] if len(c)) for b in range(m)] + [0]
    best = {"n": 0, "nis": 0.0, "asg": [-1] * m}

    def walk(b, q, used, asg, nis):
        if b == m:
            return
        for c, l in enumerate(cands[b]):
            if l in used or len(q) + 1 + rem[b] < best["n"]:
                continue
            q2 = q + [start[b] + c]
            v = float(e[q2] @ np.linalg.solve(S[np.ix_(q2, q2)], e[q2]))
            if not (np.isfinite(v) and v <= gate[len(q2) - 1]):
                continue
            a2 = asg + [l]
            if (len(q2), -v) > (best["n"], -best["nis"]):
                best.update(n=len(q2), nis=v, asg=a2 + [-1] * (m - b - 1))
            walk(b + 1, q2, used | {l}, a2, v)
        if len(q) + rem[b] >= best["n"]:
            walk(b + 1, q, used, asg + [-1], nis)

    walk(0, [], frozenset(), [], 0.0)
    return np.array(best["asg"], dtype=np.int32)


def frames_of(P, S, state, rng, poses, m, k):
    """One frame per pose: m bearings to landmarks the pose observes (repeated cyclically when it sees fewer), lists
    of the k best landmarks inside the single gate."""
    pose_xyt, lm_xy = state
    frames = []
    for a in poses:
        seen = np.unique(P.b_lm[P.b_pose == a])
        lms = np.resize(seen, m) if len(seen) < m else rng.choice(seen, m, replace=False)
        z = bearing(pose_xyt, lm_xy, np.full(m, a), lms) + 0.02 * rng.standard_normal(m)
        pose, om = np.full(m, a, dtype=np.int32), np.full(m, OMEGA)
        cl = S.associate_bearings(pose, z, om, gate=GATES[0], k=k)["cand_landmark"]
        frames.append((pose, z, om, [[int(l) for l in row if l >= 0] for row in cl]))
    return frames


def report(say, which, what, S, frames):
    new_call = lambda: S.jcbb(frames, GATES)
    t0 = time.perf_counter()
    new = new_call()
    first = 1e3 * (time.perf_counter() - t0)
    w_new, t = timed(new_call, lambda: {k: v for k, v in S.jcbb_timing().items() if k != "nodes"})
    nodes = S.jcbb_timing()["nodes"]
    pairings = int(new["cand_start"][-1])
    say(f"{which} {what}: {len(frames)} frames, {pairings} pairings; new route (solver_info {new['solver_info']}, first call {first:.1f} ms): "
        f"wall {w_new:.3f} ms = prepare+upload {t['prepare_ms']:.3f} + J+H {t['jh_ms']:.3f} + factor {t['factor_ms']:.3f} + path solve "
        f"{t['path_ms']:.3f} + products {t['product_ms']:.3f} + assembly+search kernel {t['search_ms']:.3f} + download {t['download_ms']:.3f}; "
        f"nodes per frame min {int(nodes.min())} median {int(np.median(nodes))} max {int(nodes.max())}; paired {int(new['n_paired'].sum())} of "
        f"{len(new['assignment'])} bearings; complete {int(new['complete'].sum())} of {len(frames)}; buffers {int(t['jcbb_bytes'])} bytes")
    hyps = []
    for pose, z, om, cands in frames:
        n = [len(c) for c in cands]
        hyps.append((np.repeat(pose, n), np.array([l for c in cands for l in c], dtype=np.int32), np.repeat(z, n), np.repeat(om, n)))
    host_ms, res = {"a": [], "b": []}, {}

    def old_call(route):
        out = S.joint_compatibility(hyps, cov=True)
        t1 = time.perf_counter()
        asg = []
        for f, (_, _, _, cands) in enumerate(frames):
            q = slice(out["hyp_start"][f], out["hyp_start"][f + 1])
            if route == "a":
                asg.append(bos.jcbb_search_host(cands, out["innovation_cov"][f], out["innovation"][q], GATES)["assignment"])
            else:
                asg.append(numpy_search(cands, out["innovation_cov"][f], out["innovation"][q], GATES))
        host_ms[route].append(1e3 * (time.perf_counter() - t1))
        res[route] = np.concatenate(asg)

    for route, name in (("a", "joint_compatibility(cov) + compiled serial search"), ("b", "joint_compatibility(cov) + NumPy search")):
        # the NumPy search takes 0.1 - 0.5 s per frame: fewer repetitions where it would run for minutes
        w_old, tj = timed(lambda: old_call(route), S.joint_compatibility_timing, 10 if route == "a" else (3 if len(frames) == 1 else 1))
        same = bool(np.array_equal(res[route], new["assignment"]))
        say(f"{which} {what}: old route {route} ({name}): wall {w_old:.3f} ms = joint call {w_old - float(np.median(host_ms[route][1:])):.3f} "
            f"(NIS kernel {tj['nis_ms']:.3f}, download {tj['download_ms']:.3f}) + host search {float(np.median(host_ms[route][1:])):.3f}; "
            f"downloads {8 * sum(len(h[0]) ** 2 + 3 * len(h[0]) + 1 for h in hyps)} bytes against {4 * len(new['assignment']) + 24 * len(frames)}; "
            f"new / old {w_new / w_old:.3f}, old / new {w_old / w_new:.2f}; same assignment {same}")


def measure(which, say):
    P = problem(which)
    S = bos.Solver(P, device=0)
    S.step()
    state = S.get_state()
    rng = np.random.default_rng(43)
    say(f"{which}: NP {P.NP} NL {P.NL} n {S.system_info()['n']}")
    free = np.array([p for p in range(max(0, P.NP - 4000), P.NP) if p != P.fixed])
    observing = np.unique(P.b_pose[np.isin(P.b_pose, free)])
    counts = np.array([len(np.unique(P.b_lm[P.b_pose == p])) for p in observing])
    rich = observing[np.argsort(-counts, kind="stable")]
    report(say, which, "one8x4", S, frames_of(P, S, state, rng, rich[:1], 8, 4))
    report(say, which, "one16x2", S, frames_of(P, S, state, rng, rich[:1], 16, 2))
    report(say, which, "many8x4", S, frames_of(P, S, state, rng, rich[:64], 8, 4))
    S.close()


def base(which, lib):
    """step() and joint_compatibility() (256 hypotheses of 8) alone: wall ms, medians of 10 after a warm-up."""
    if lib:
        bos.LIB_PATH = os.path.abspath(lib)
        bos.ALLOW_MISSING_SYMBOLS = True
    P = problem(which)
    S = bos.Solver(P, device=0)
    S.step()
    rng = np.random.default_rng(29)
    free = np.array([p for p in range(max(0, P.NP - 4000), P.NP) if p != P.fixed])
    a = int(free[-1])
    lm = rng.integers(0, P.NL, 8 * 256).astype(np.int32)
    z = rng.uniform(-3, 3, 8 * 256)
    start = 8 * np.arange(257, dtype=np.int32)
    w_j, _ = timed(lambda: S.joint_compatibility((start, np.full(8 * 256, a, dtype=np.int32), lm), z, np.full(8 * 256, OMEGA)),
                   S.joint_compatibility_timing)
    S.step()
    steps = []
    for _ in range(10):
        t0 = time.perf_counter()
        S.step()
        steps.append(1e3 * (time.perf_counter() - t0))
    print(f"{which} {'other' if lib else 'this '}: joint_compatibility {w_j:.3f}  step {float(np.median(steps)):.3f}", flush=True)
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
                for key, x in zip(("joint_compatibility", "step"), v):
                    seen.setdefault((which, key, other), []).append(x)
    print()
    for (which, key, other), v in sorted(seen.items()):
        print(f"{which} {key:19s} {'other' if other else 'this '}: min {min(v):.3f} median {float(np.median(v)):.3f} max {max(v):.3f} ms "
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
    out = args[1] if len(args) > 1 and args[0] == "--out" else os.path.join(ROOT, "profiles", "r16_jcbb.txt")
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
