"""Time of an LM iteration (bos_optimize) beside the GN step of the same handle (measurement, not a
test):

    python3 tools/lm_time.py            # c1, c2, c3
    python3 tools/lm_time.py c2         # one problem alone (c1 | c2 | c3)

Without an argument every problem runs as a child process of its own under its own time limit, and
the first one that fails ends the run.

Per problem and precision, on one handle after a warm-up (graphs captured, buffers allocated), medians
of 5: ms per GN step from bos_time_steps (synchronous steps) and from step_n(K) (one batch); ms per LM
iteration from optimize(lambda0=0.01, max_iterations=K, tolerances 0) with check_every 1 (a host read per
iteration, as bos_step) and check_every K (one batch), divided by K; the cost kernel alone and the
J+H build alone (back to back, HIP events). Every timed call starts from the initial guess
(set_state outside the timed region). The yardstick of an LM iteration is the GN step of the
same kind (synchronous / batched): it adds one fp64 cost pass, five small launches and the backup."""
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "prb-project-bearing-only-slam_amd"))
import bos  # noqa: E402

LIMITS = {"c1": 120, "c2": 120, "c3": 420}
K = 10
LAMBDA0 = 0.01   # the GN steps' damping factor: the first LM iteration is that step


def problem(which):
    if which == "c1":
        return bos.load_g2o(os.path.join(ROOT, "tests", "golden", "data", "slam2D_bearing_only_initial_guess.g2o"))
    return bos.synthetic(1000, 2000, 20) if which == "c2" else bos.synthetic(100000, 200000, 10)


def wall(f):
    t0 = time.perf_counter()
    r = f()
    return 1e3 * (time.perf_counter() - t0), r


def measure(which):
    P = problem(which)
    for prec in (bos.BOS_FP64, bos.BOS_FP32):
        S = bos.Solver(P, device=0, precision=prec)
        init = S.get_state()
        S.step_n(2)
        S.optimize(lambda0=LAMBDA0, max_iterations=2, dx_tol=0.0, f_tol=0.0)

        def from_init(f):   # every timed call starts at the initial guess: K iterations that move the state
            S.set_state(*init)
            S.synchronize()
            return wall(f)

        gn_sync = float(np.median([from_init(lambda: S.time_steps(K))[1] for _ in range(5)]))
        gn_batch = float(np.median([from_init(lambda: S.step_n(K))[0] / K for _ in range(5)]))
        lm_sync, lm_batch, flags = [], [], []
        for every, out in ((1, lm_sync), (K, lm_batch)):
            for _ in range(5):
                ms, r = from_init(lambda: S.optimize(lambda0=LAMBDA0, max_iterations=K, check_every=every, dx_tol=0.0, f_tol=0.0))
                assert r["iterations"] == K and r["reason"] == 3, r
                out.append(ms / K)
                flags.append(r["accepted"])
        cost = S.time_cost(50)
        jh = S.time_linearize(50)
        lm_sync, lm_batch = float(np.median(lm_sync)), float(np.median(lm_batch))
        tag = f"{which} fp{prec}"
        print(f"{tag}: NP {P.NP} NL {P.NL} bearings {len(P.b_z)} n {S.system_info()['n']}")
        print(f"{tag}: GN step {gn_sync:.4f} ms synchronous, {gn_batch:.4f} ms in a batch of {K}")
        print(f"{tag}: LM iteration {lm_sync:.4f} ms with check_every 1 ({lm_sync - gn_sync:+.4f} ms, x{lm_sync / gn_sync:.3f}), "
              f"{lm_batch:.4f} ms with check_every {K} ({lm_batch - gn_batch:+.4f} ms, x{lm_batch / gn_batch:.3f}); "
              f"accepted of {K} per call {flags}")
        print(f"{tag}: cost kernel {cost:.4f} ms, J+H build {jh:.4f} ms (back to back, warm)", flush=True)
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
