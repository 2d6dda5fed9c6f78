"""Timing of the prior kernel's cost at config 3 (fp32, SCHUR): time_steps / time_linearize without priors, with
priors on all landmarks, with priors on every free node. --lib PATH loads another build (the parent's) for the
no-priors line. One line per measurement on stdout (profiles/r18_priors.txt)."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "prb-project-bearing-only-slam_amd"))
import bos  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--lib", default=None)
ap.add_argument("--tag", default="this")
ap.add_argument("--priors", action="store_true")
ap.add_argument("--n", type=int, default=200)
ap.add_argument("--reps", type=int, default=3)
a = ap.parse_args()
if a.lib:
    bos.LIB_PATH = a.lib
    bos.ALLOW_MISSING_SYMBOLS = True
import numpy as np  # noqa: E402

P = bos.synthetic(100000, 200000, 10)


def measure(label, setup):
    S = bos.Solver(P, precision=bos.BOS_FP32, solver=bos.BOS_SOLVER_SCHUR)
    setup(S)
    S.time_steps(20)
    S.time_linearize(20)
    for r in range(a.reps):
        S.set_state(P.pose_xyt, P.lm_xy)
        ts = S.time_steps(a.n)
        st = S.step()
        assert st["solver_info"] == 0 and st["max_abs_dx"] < 0.05, st   # the timed iteration converged
        S.set_state(P.pose_xyt, P.lm_xy)
        tl = S.time_linearize(a.n)
        tc = S.time_linearize(50, flush_caches=True)
        print(f"{a.tag} | {label} | rep {r} | step {ts * 1e3:.1f} us | linearize back-to-back {tl * 1e3:.2f} us | "
              f"linearize cold {tc * 1e3:.2f} us", flush=True)
    S.close()


measure("no priors", lambda S: None)
if a.priors:
    # means at the estimate the edges alone converge to (so sum rho is about 0): the priors agree with the data and
    # the timed GN iteration stays the converging one that is timed without priors; profiles/r18_priors.txt records
    # what priors at noisy positions did to the timing instead
    S0 = bos.Solver(P, precision=bos.BOS_FP32, solver=bos.BOS_SOLVER_SCHUR)
    S0.step_n(30)
    pose_c, lm_c = S0.get_state()
    S0.close()
    li = np.arange(P.NL, dtype=np.int32)
    lmp = (li, lm_c, np.tile(100.0 * np.eye(2), (P.NL, 1, 1)))
    free = np.array([p for p in range(P.NP) if p != P.fixed], dtype=np.int32)
    pp = (free, pose_c[free], np.tile(np.diag([100.0, 100.0, 1000.0]), (len(free), 1, 1)))
    measure("priors on all 200000 landmarks", lambda S: S.set_priors(landmark=lmp))
    measure("priors on every free node (99999 poses + 200000 landmarks)", lambda S: S.set_priors(pose=pp, landmark=lmp))
