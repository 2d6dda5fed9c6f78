"""Reference of the Levenberg-Marquardt tests (test_lm_host.py, test_gpu_lm.py): pure Python on the
CPU oracle, no code shared with the product.

Objective. F(x) = sum over all edges (bearings and odometry, self-loops included) of h(rho),
rho = e^T Omega e, h(rho) = rho for rho <= kt and 2 sqrt(kt rho) - kt beyond: the function whose half
gradient the reference's robust J+H builds. Errors from O.bearing_errors and
O.odometry_error_and_jacobian.

One iteration at (x, lambda): O.linearize(damping=lambda) -> solve -> O.apply_boxplus -> F, then the
rule below. The solve is done twice, by O.solve_dx (sparse LU of the reduced system) and by a dense
Cholesky of the same matrix; what the two give differs by the rounding of two direct fp64 solves
with different elimination orders, and that per-iteration disagreement is the yardstick the
tolerances of the GPU comparison are multiples of (`disagreement`)."""
import types

import numpy as np
import scipy.linalg as sla

import oracle as O

DEFAULTS = dict(lambda0=0.0, lambda_min=1e-12, lambda_max=1e12, dx_tol=1e-6, f_tol=1e-12, max_iterations=50,
                check_every=4)


def huber(rho, kt):
    rho = np.asarray(rho, dtype=np.float64)
    return np.where(rho <= kt, rho, 2.0 * np.sqrt(kt * rho) - kt)


def edge_rhos(Q, pose, lm):
    """rho of every bearing, then of every odometry edge, at a state."""
    e = O.bearing_errors(Q, pose, lm)
    w = 1.0 if Q.b_omega is None else np.asarray(Q.b_omega, dtype=np.float64)
    rb = e * w * e
    ro = np.zeros(len(Q.o_z))
    for k in range(len(Q.o_z)):
        eo, _ = O.odometry_error_and_jacobian(pose[Q.o_src[k]], pose[Q.o_dst[k]], Q.o_z[k])
        ro[k] = eo @ np.asarray(Q.o_omega[k], dtype=np.float64).reshape(3, 3) @ eo
    return rb, ro


def cost(Q, pose, lm, kt):
    """(F, chi2, n_robust) at a state."""
    rb, ro = edge_rhos(Q, np.ascontiguousarray(pose, dtype=np.float64), np.ascontiguousarray(lm, dtype=np.float64))
    rho = np.concatenate([rb, ro])
    return float(huber(rho, kt).sum()), float(rho.sum()), int((rho > kt).sum())


def options(**kw):
    o = dict(DEFAULTS)
    for k, v in kw.items():
        assert k in o, k
        o[k] = v
    return o


def new_state(lam, F, nu=2.0):
    return dict(iteration=0, accepted=0, rejected=0, done=0, reason=0, cost=float(F), nu=float(nu), **{"lambda": float(lam)})


def rule(st, o, cost_trial, predicted, max_dx, solver_info=0):
    """The issue's step 5 and 6 on a copy of st: (state, record, counted)."""
    st = dict(st)
    if st["done"]:
        return st, dict(accepted=0), False
    F, lam = st["cost"], st["lambda"]
    ok = solver_info == 0 and predicted > 0.0 and bool(np.isfinite(cost_trial))
    gain = (F - cost_trial) / predicted if ok else 0.0
    accept = ok and gain > 0.0
    at_max = lam >= o["lambda_max"]
    if accept:
        t = 2.0 * gain - 1.0
        st["lambda"] = lam * max(1.0 / 3.0, 1.0 - t * t * t)
        st["nu"] = 2.0
        st["cost"] = float(cost_trial)
        st["accepted"] += 1
    else:
        st["lambda"] = lam * st["nu"]
        st["nu"] = 2.0 * st["nu"]
        st["rejected"] += 1
    st["lambda"] = min(max(st["lambda"], o["lambda_min"]), o["lambda_max"])
    st["iteration"] += 1
    if o["dx_tol"] > 0.0 and max_dx <= o["dx_tol"]:
        st["reason"] = 1
    elif accept and o["f_tol"] > 0.0 and F - cost_trial <= o["f_tol"] * F:
        st["reason"] = 2
    elif not accept and at_max:
        st["reason"] = 4
    elif st["iteration"] >= o["max_iterations"]:
        st["reason"] = 3
    st["done"] = int(st["reason"] != 0)
    rec = dict(cost=F, cost_trial=float(cost_trial), predicted=float(predicted), gain=float(gain), max_abs_dx=float(max_dx),
               solver_info=int(solver_info), accepted=int(accept), **{"lambda": lam})
    return st, rec, True


def solve_dense(Q, H, b):
    """The reduced system by dense Cholesky: dx with the fixed pose's zeros re-inserted."""
    Hnf, bnf, idx = O.reduced_system(Q, H, b)
    c = sla.cho_factor(Hnf.toarray(), lower=True)
    dx = np.zeros(Q.N)
    dx[idx] = sla.cho_solve(c, -bnf)
    return dx


def trial(Q, pose, lm, kt, lam, dx, b):
    """(predicted, F', trial pose, trial landmarks) of an update."""
    pred = float(dx @ (lam * dx - b))
    p, l = pose.copy(), lm.copy()
    O.apply_boxplus(Q, p, l, dx)
    return pred, cost(Q, p, l, kt)[0], p, l


def iterate(Q, pose, lm, kt, st, o, dense=True):
    """One LM iteration from (pose, lm) with the state st (its cost must be F at that state).
    Returns a namespace: st (new state), rec, counted, pose / lm (the iterate afterwards), dx,
    trial_pose / trial_lm, and with dense=True the second solve's rec_d / dx_d and `dis`, the
    disagreement of the two solves (dx: max abs; cost_trial, predicted: relative; gain: absolute)."""
    pose = np.ascontiguousarray(pose, dtype=np.float64)
    lm = np.ascontiguousarray(lm, dtype=np.float64)
    lam = st["lambda"]
    lin = O.linearize(Q, pose, lm, kernel_threshold=kt, damping=lam)
    H = O.assemble_H(Q, lin)
    keep = np.ones(Q.N, dtype=bool)
    keep[3 * Q.fixed:3 * Q.fixed + 3] = False
    b = np.where(keep, lin.b, 0.0)
    dx = O.solve_dx(Q, H, lin.b)
    pred, Ft, tp, tl = trial(Q, pose, lm, kt, lam, dx, b)
    st2, rec, counted = rule(st, o, Ft, pred, float(np.abs(dx).max()))
    out = types.SimpleNamespace(st=st2, rec=rec, counted=counted, dx=dx, trial_pose=tp, trial_lm=tl,
                                pose=tp if rec["accepted"] else pose, lm=tl if rec["accepted"] else lm)
    if dense:
        dxd = solve_dense(Q, H, lin.b)
        pd, Fd, _, _ = trial(Q, pose, lm, kt, lam, dxd, b)
        _, recd, _ = rule(st, o, Fd, pd, float(np.abs(dxd).max()))
        out.dx_d, out.rec_d = dxd, recd
        out.dis = dict(dx=float(np.abs(dx - dxd).max()), cost_trial=abs(Ft - Fd) / max(abs(Ft), 1e-300),
                       predicted=abs(pred - pd) / max(abs(pred), 1e-300), gain=abs(rec["gain"] - recd["gain"]))
    return out


def run(Q, pose, lm, kt, o, dense=False):
    """The loop from (pose, lm): (final pose, lm, state, list of iterate() results)."""
    pose = np.ascontiguousarray(pose, dtype=np.float64).copy()
    lm = np.ascontiguousarray(lm, dtype=np.float64).copy()
    lam = o["lambda0"] if o["lambda0"] > 0.0 else 0.01
    st = new_state(lam, cost(Q, pose, lm, kt)[0])
    its = []
    while not st["done"]:
        it = iterate(Q, pose, lm, kt, st, o, dense=dense)
        st, pose, lm = it.st, it.pose, it.lm
        its.append(it)
    return pose, lm, st, its


def perturbed_poses(P):
    """The issue's "perturbed" input: poses + default_rng(2).normal(size=(NP, 3)) * [1, 1, 0.5], the
    fixed pose untouched."""
    d = np.random.default_rng(2).normal(size=(P.NP, 3)) * np.array([1.0, 1.0, 0.5])
    d[P.fixed] = 0.0
    return P.pose_xyt + d


def recovered_dx(pose0, lm0, pose1, lm1):
    """The update that took (pose0, lm0) to (pose1, lm1) by the left box-plus: per pose
    (x1 - R(dth) x0, wrapped dth), per landmark the difference."""
    dth = (pose1[:, 2] - pose0[:, 2] + np.pi) % (2 * np.pi) - np.pi
    c, s = np.cos(dth), np.sin(dth)
    dxy = pose1[:, :2] - np.stack([c * pose0[:, 0] - s * pose0[:, 1], s * pose0[:, 0] + c * pose0[:, 1]], axis=1)
    return np.concatenate([np.column_stack([dxy, dth]).ravel(), (lm1 - lm0).ravel()])


def with_poses(P, pose_xyt):
    """A copy of the product's problem P (bos.Problem) with other initial poses."""
    return type(P)(pose_xyt, P.lm_xy, P.b_pose, P.b_lm, P.b_z, P.o_src, P.o_dst, P.o_z, P.o_omega, P.fixed,
                   b_omega=P.b_omega, pose_ids=P.pose_ids, lm_ids=P.lm_ids)


def assert_comparable(it):
    """The issue's conditions on a reference iteration before anything is compared with it."""
    r = it.rec
    assert abs(r["gain"]) >= 0.05, r
    assert r["predicted"] >= 1e-3 * r["cost"], r


def check_iteration(tag, rec, before, after, lam_next, it, flags_only=False):
    """One iteration of the code under test (trace record rec, state before / after as (pose, lm),
    lambda afterwards) against the reference iteration `it` started from the same state and lambda.
    Tolerances: max(floor, 100 x the two reference solves' disagreement of this iteration); floors
    1e-9 relative (costs, predicted), 1e-9 absolute (gain), 1e-6 max |dx| (update). The next lambda is
    lambda f(gain): its bound is the gain's bound through |df/dgain| = 6 (2 gain - 1)^2 (plus 1e-12
    relative for the products' rounding). Returns {quantity: error / tolerance}."""
    r, d = it.rec, it.dis
    assert rec["accepted"] == r["accepted"], (tag, rec, r)
    assert rec["solver_info"] == 0, (tag, rec)
    if flags_only:
        assert abs(rec["gain"] - r["gain"]) <= 1e-3, (tag, rec["gain"], r["gain"])
        return {}
    maxdx = float(np.abs(it.dx).max())
    tol = dict(cost=1e-9, cost_trial=max(1e-9, 100 * d["cost_trial"]), predicted=max(1e-9, 100 * d["predicted"]),
               gain=max(1e-9, 100 * d["gain"]), dx=max(1e-6 * maxdx, 100 * d["dx"]))
    err = dict(cost=abs(rec["cost"] - r["cost"]) / abs(r["cost"]),
               cost_trial=abs(rec["cost_trial"] - r["cost_trial"]) / abs(r["cost_trial"]),
               predicted=abs(rec["predicted"] - r["predicted"]) / abs(r["predicted"]),
               gain=abs(rec["gain"] - r["gain"]))
    assert rec["lambda"] == r["lambda"], (tag, rec["lambda"], r["lambda"])
    if r["accepted"]:
        err["dx"] = float(np.abs(recovered_dx(before[0], before[1], after[0], after[1]) - it.dx).max())
        t = 2.0 * r["gain"] - 1.0
        tol["lambda_next"] = (r["lambda"] * 6.0 * t * t * tol["gain"] + 1e-12 * it.st["lambda"]) / it.st["lambda"]
    else:
        assert np.array_equal(before[0], after[0]) and np.array_equal(before[1], after[1]), tag
        err["dx"] = abs(rec["max_abs_dx"] - maxdx)
        tol["lambda_next"] = 1e-12
    err["lambda_next"] = abs(lam_next - it.st["lambda"]) / it.st["lambda"]
    ratio = {k: err[k] / tol[k] for k in tol}
    print(f"{tag}: acc {r['accepted']} gain {r['gain']:.3f} lambda {r['lambda']:.3g} err/tol " +
          " ".join(f"{k} {v:.3g}" for k, v in ratio.items()))
    bad = {k: (err[k], tol[k]) for k in tol if not err[k] <= tol[k]}
    assert not bad, (tag, bad)
    return ratio
