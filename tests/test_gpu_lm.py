"""Solver.cost() / Solver.optimize() (bos_cost, bos_optimize: Levenberg-Marquardt with the step
control on the device) against the oracle reference of tests/lm_ref.py, against the GN step the first
iteration must reproduce, against itself (batched / single, rollback) and against the CPU twin.

Inputs (the issue's): "plain" = the dataset's initial guess, kt 1, lambda0 0.01; "perturbed" = its
poses + default_rng(2) normal * [1, 1, 0.5], kt 1e30, lambda0 1e-4, 14 iterations (A A A A r r r r A
A A A A A on the oracle). Tolerances of the one-step parity: lm_ref.check_iteration."""
import numpy as np
import pytest

import bos
import lm_ref as R
import oracle as O
from conftest import C1
from helpers import knife_edge_bearings, to_oracle

pytestmark = pytest.mark.gpu

SCHUR, SUPERNODAL = bos.BOS_SOLVER_SCHUR, bos.BOS_SOLVER_SUPERNODAL
FP64, FP32 = bos.BOS_FP64, bos.BOS_FP32
NOTOL = dict(dx_tol=0.0, f_tol=0.0)


@pytest.fixture(scope="module")
def c1():
    return bos.load_g2o(C1)


@pytest.fixture(scope="module")
def pert(c1):
    P = R.with_poses(c1, R.perturbed_poses(c1))
    return P, to_oracle(P)


@pytest.fixture(scope="module")
def plain_ref(c1):
    """The reference loop on "plain" with dx_tol 1e-4: (state, iterations)."""
    Q = to_oracle(c1)
    _, _, st, its = R.run(Q, Q.pose_xyt, Q.lm_xy, 1.0, R.options(lambda0=0.01, dx_tol=1e-4))
    return st, its


@pytest.fixture(scope="module")
def pert_ref(pert):
    """The reference loop on "perturbed", 14 iterations, with its own preconditions checked."""
    P, Q = pert
    S = bos.Solver(P, kernel_threshold=1e30)   # the state as a handle holds it (theta wrapped)
    pose, lm = S.get_state()
    S.close()
    _, _, st, its = R.run(Q, pose, lm, 1e30, R.options(lambda0=1e-4, max_iterations=14, **NOTOL), dense=True)
    flags = [it.rec["accepted"] for it in its]
    assert len(flags) == 14 and flags.count(0) >= 2 and flags.count(1) >= 5, flags
    for it in its:
        R.assert_comparable(it)
    return st, its, flags


def _no_knife_edge(P, pose, lm):
    Q = to_oracle(R.with_poses(P, pose))
    Q.lm_xy = np.ascontiguousarray(lm).copy()
    assert len(knife_edge_bearings(Q)[0]) == 0


def _rec(tr, i=0):
    return {k: tr[i][k].item() for k in tr.dtype.names}


def _same(a, b):
    return np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


# ---------------------------------------------------------------- 1. cost parity
@pytest.mark.parametrize("precision", [FP64, FP32])
@pytest.mark.parametrize("steps", [0, 3])
def test_cost_parity(c1, precision, steps):
    S = bos.Solver(c1, precision=precision)
    if steps:
        S.step_n(steps)
    pose, lm = S.get_state()
    Q = to_oracle(c1)
    for kt in (1.0, 1e30, 1e-3):
        S.set_kernel_threshold(kt)
        got = S.cost()
        F, chi, nrob = R.cost(Q, pose, lm, kt)
        print(f"cost fp{precision} after {steps} steps kt {kt:g}: F {got['cost']:.12g} ref {F:.12g} rel "
              f"{abs(got['cost'] - F) / F:.2e} chi2 rel {abs(got['chi2'] - chi) / chi:.2e} robust {got['n_robust']}")
        assert abs(got["cost"] - F) <= 1e-9 * F
        assert abs(got["chi2"] - chi) <= 1e-9 * chi
        assert got["n_robust"] == nrob
        if kt == 1e30:
            chi_lin = S.linearize()["chi2"]
            assert abs(got["cost"] - chi_lin) <= (1e-9 if precision == FP64 else 1e-3) * chi_lin
    assert _same(S.get_state(), (pose, lm))
    S.close()


# ---------------------------------------------------------------- 2. cost edge shapes
def _world(NP, NL, per_pose, seed, weights=False):
    """A small world: poses on a noisy arc, landmarks around it, per_pose bearings per pose (none for
    pose 5), an odometry chain with per-edge SPD information (off-diagonals included)."""
    rng = np.random.default_rng(seed)
    t = np.linspace(0.0, 4.0, NP)
    gt = np.column_stack([6 * np.cos(t), 6 * np.sin(t), t + np.pi / 2])
    pose = gt + rng.normal(0, 0.05, (NP, 3))
    lm = rng.uniform(-9, 9, (NL, 2))
    bp, bl = [], []
    for p in range(NP):
        if p == 5:
            continue
        for l in rng.choice(NL, min(per_pose, NL), replace=False):
            bp.append(p)
            bl.append(l)
    for l in range(NL):   # every landmark seen (the last one exactly once when per_pose leaves it out)
        if l not in bl:
            bp.append(0)
            bl.append(l)
    bp, bl = np.array(bp, dtype=np.int32), np.array(bl, dtype=np.int32)
    c, s = np.cos(gt[bp, 2]), np.sin(gt[bp, 2])
    d = lm[bl] - gt[bp, :2]
    z = np.arctan2(-s * d[:, 0] + c * d[:, 1], c * d[:, 0] + s * d[:, 1]) + rng.normal(0, 0.02, len(bp))
    z = (z + np.pi) % (2 * np.pi) - np.pi
    src = np.arange(NP - 1, dtype=np.int32)
    dst = src + 1
    oz = np.array([O.predict_odometry(gt[a], gt[b]) for a, b in zip(src, dst)]) + rng.normal(0, 0.02, (NP - 1, 3))
    A = rng.normal(0, 1, (NP - 1, 3, 3))
    om = 50.0 * (A @ A.transpose(0, 2, 1) + np.eye(3))
    w = rng.uniform(0.5, 2.0, len(z)) if weights else None
    return bos.Problem(pose, lm, bp, bl, z, src, dst, oz, om, 0, b_omega=w, pose_ids=np.arange(NP, dtype=np.int32),
                       lm_ids=np.arange(NL, dtype=np.int32))


def _hand_built():
    """12 poses, 6 landmarks: pose 5 without bearings, landmark 5 seen once, bearing weights, the pair
    (pose 2, landmark 1) twice, a reversed edge (4 -> 3), a loop closure (0 -> 9), a self-loop (7, 7)
    with rho above the threshold, per-edge SPD information with off-diagonals."""
    P = _world(12, 6, 3, seed=11, weights=True)
    keep = P.b_lm != 5
    keep[np.nonzero(~keep)[0][:1]] = True   # landmark 5: its first observation only
    bp, bl, bz, bw = P.b_pose[keep], P.b_lm[keep], P.b_z[keep], P.b_omega[keep]
    bp, bl = np.append(bp, [2, 2]).astype(np.int32), np.append(bl, [1, 1]).astype(np.int32)
    bz, bw = np.append(bz, [0.3, 0.31]), np.append(bw, [1.5, 0.7])
    src = np.append(P.o_src, [4, 0, 7]).astype(np.int32)
    dst = np.append(P.o_dst, [3, 9, 7]).astype(np.int32)
    Q = to_oracle(P)
    oz = np.concatenate([P.o_z, [O.predict_odometry(Q.pose_xyt[4], Q.pose_xyt[3]) + 0.02,
                                 O.predict_odometry(Q.pose_xyt[0], Q.pose_xyt[9]) - 0.03, [2.0, -1.0, 0.5]]])
    om = np.concatenate([P.o_omega, P.o_omega[:3]])
    return bos.Problem(P.pose_xyt, P.lm_xy, bp, bl, bz, src, dst, oz, om, 0, b_omega=bw, pose_ids=P.pose_ids, lm_ids=P.lm_ids)


@pytest.mark.parametrize("precision", [FP64, FP32])
@pytest.mark.parametrize("shape", ["hand_lpp1", "hand_lpp2", "hand_lpp4", "np65_nl257"])
def test_cost_edge_shapes(shape, precision):
    """The cost on hand-built problems (each edge once, self-loops included), and one past a wave of
    poses / one past a block of landmarks; then one LM iteration on the same handle against the GN
    step it must reproduce (the damping kernel on duplicate pairs and 1, 2, 4 lanes per pose)."""
    P = _hand_built() if shape.startswith("hand") else _world(65, 257, 8, seed=12)
    lpp = int(shape[-1]) if shape.startswith("hand") else 0
    Q = to_oracle(P)
    S = bos.Solver(P, precision=precision, lanes_per_pose=lpp)
    pose, lm = S.get_state()
    for kt in (1.0, 1e-3, 1e30):
        S.set_kernel_threshold(kt)
        got = S.cost()
        F, chi, nrob = R.cost(Q, pose, lm, kt)
        print(f"cost {shape} fp{precision} kt {kt:g}: rel {abs(got['cost'] - F) / F:.2e} robust {nrob}")
        assert abs(got["cost"] - F) <= 1e-9 * F and abs(got["chi2"] - chi) <= 1e-9 * chi and got["n_robust"] == nrob
    S.set_kernel_threshold(1.0)
    G = bos.Solver(P, precision=precision, lanes_per_pose=lpp, damping=0.05)
    G.step()
    r = S.optimize(lambda0=0.05, max_iterations=1, **NOTOL)
    assert r["trace"]["solver_info"][0] == 0
    if r["trace"]["accepted"][0]:
        assert _same(S.get_state(), G.get_state())
    else:
        assert _same(S.get_state(), (pose, lm))
    assert r["trace"]["max_abs_dx"][0] == G.last_stats["max_abs_dx"]
    S.close()
    G.close()


# ---------------------------------------------------------------- 3. the first iteration is a GN step
@pytest.mark.parametrize("precision", [FP64, FP32])
@pytest.mark.parametrize("solver", [SCHUR, SUPERNODAL])
@pytest.mark.parametrize("d", [0.01, 1e-3])
def test_first_iteration_is_a_gn_step(c1, plain_ref, precision, solver, d):
    assert plain_ref[1][0].rec["accepted"] == 1
    G = bos.Solver(c1, precision=precision, solver=solver, damping=d)
    st = G.step()
    S = bos.Solver(c1, precision=precision, solver=solver)
    r = S.optimize(lambda0=d, max_iterations=1, **NOTOL)
    assert r["iterations"] == 1 and r["accepted"] == 1 and r["reason"] == 3
    assert _same(S.get_state(), G.get_state())
    assert r["trace"]["max_abs_dx"][0] == st["max_abs_dx"] and r["trace"]["lambda"][0] == d
    # export_system gives the iteration's damped system: the step's, bit for bit
    es, eg = S.export_system(), G.export_system()
    assert np.array_equal(es[2], eg[2]) and np.array_equal(es[3], eg[3])
    with pytest.raises(bos.BosError, match=r"\(-1\)"):
        S.last_dx()
    S.close()
    G.close()


# ---------------------------------------------------------------- 4. one-step parity on "perturbed"
@pytest.mark.parametrize("kind", ["fp64_schur", "fp64_supernodal", "fp32_schur"])
def test_one_step_parity_perturbed(pert, pert_ref, kind):
    """Fourteen single iterations, each against one reference iteration from the handle's own previous
    state and lambda (no error compounds). fp32: the flags, and the gain to 1e-3. Measured on an
    MI355X, worst error / tolerance over the 14 iterations: fp64 Schur cost 2e-7, cost_trial 0.022,
    predicted 1.1e-3, gain 4.8e-3, dx 1.8e-3, next lambda 4e-3; fp64 supernodal 4e-7, 0.014, 1.1e-3,
    4.1e-3, 2e-3, 1.7e-3."""
    P, Q = pert
    kt = 1e30
    fp32 = kind.startswith("fp32")
    S = bos.Solver(P, precision=FP32 if fp32 else FP64, solver=SUPERNODAL if kind.endswith("supernodal") else SCHUR,
                   kernel_threshold=kt)
    o = R.options(max_iterations=1, **NOTOL)
    lam, nu, flags, worst = 1e-4, 2.0, [], {}
    for i in range(14):
        before = S.get_state()
        _no_knife_edge(P, *before)
        r = S.optimize(lambda0=1e-4 if i == 0 else 0.0, max_iterations=1, **NOTOL)
        after = S.get_state()
        assert r["iterations"] == 1 and r["reason"] == 3 and len(r["trace"]) == 1
        rec = _rec(r["trace"])
        it = R.iterate(Q, before[0], before[1], kt, R.new_state(lam, R.cost(Q, before[0], before[1], kt)[0], nu), o)
        R.assert_comparable(it)
        _no_knife_edge(P, it.trial_pose, it.trial_lm)
        for k, v in R.check_iteration(f"{kind} it {i}", rec, before, after, r["lambda_final"], it, flags_only=fp32).items():
            worst[k] = max(worst.get(k, 0.0), v)
        assert r["cost_final"] == (rec["cost_trial"] if rec["accepted"] else rec["cost"])
        flags.append(rec["accepted"])
        lam, nu = r["lambda_final"], it.st["nu"]
    S.close()
    print(f"{kind} worst err/tol:", {k: f"{v:.3g}" for k, v in worst.items()}, "flags", flags)
    assert flags.count(0) >= 2 and flags.count(1) >= 5
    if not fp32:
        assert flags == pert_ref[2]


# ---------------------------------------------------------------- 5. batched equals single
@pytest.mark.parametrize("precision", [FP64, FP32])
def test_batched_equals_single(pert, precision):
    P, _ = pert
    A = bos.Solver(P, precision=precision, kernel_threshold=1e30)
    ra = A.optimize(lambda0=1e-4, max_iterations=14, check_every=5, **NOTOL)
    B = bos.Solver(P, precision=precision, kernel_threshold=1e30)
    tr = [B.optimize(lambda0=1e-4 if i == 0 else 0.0, max_iterations=1, **NOTOL) for i in range(14)]
    assert ra["iterations"] == 14 and ra["reason"] == 3 and ra["rejected"] >= 2 and ra["accepted"] >= 5
    assert _same(A.get_state(), B.get_state())
    singles = np.concatenate([t["trace"] for t in tr])
    assert ra["trace"].tobytes() == singles.tobytes()
    assert ra["cost_final"] == tr[-1]["cost_final"] and ra["lambda_final"] == tr[-1]["lambda_final"]
    assert ra["cost_initial"] == tr[0]["cost_initial"]
    A.close()
    B.close()


# ---------------------------------------------------------------- 6. rollback is exact
@pytest.mark.parametrize("precision", [FP64, FP32])
def test_rollback_is_exact(pert, pert_ref, precision):
    P, _ = pert
    assert pert_ref[2][:5] == [1, 1, 1, 1, 0]
    S = bos.Solver(P, precision=precision, kernel_threshold=1e30)
    r = S.optimize(lambda0=1e-4, max_iterations=4, **NOTOL)
    assert r["accepted"] == 4
    state = S.get_state()
    S.linearize()
    v0, b0 = S.export_system()[2:]
    r = S.optimize(max_iterations=1, **NOTOL)
    assert r["iterations"] == 1 and r["rejected"] == 1 and r["trace"]["accepted"][0] == 0
    assert r["cost_final"] == r["cost_initial"] == r["trace"]["cost"][0]
    assert _same(S.get_state(), state)
    S.linearize()
    v1, b1 = S.export_system()[2:]
    assert np.array_equal(v0, v1) and np.array_equal(b0, b1)
    S.close()


# ---------------------------------------------------------------- 7. stops by itself
def test_stops_by_itself(c1, plain_ref):
    st, its = plain_ref
    S = bos.Solver(c1)
    r = S.optimize(lambda0=0.01, dx_tol=1e-4)
    print(f"plain: {r['iterations']} iterations (ref {st['iteration']}), reason {r['reason']}, cost {r['cost_final']:.10g} "
          f"(ref {st['cost']:.10g}), lambda {r['lambda_final']:.3g}")
    assert r["reason"] == 1 == st["reason"]
    assert r["iterations"] <= st["iteration"] + 2 and r["iterations"] < 50
    assert abs(r["cost_final"] - st["cost"]) <= 1e-6 * st["cost"]
    assert np.all(np.diff(r["trace"]["cost"]) <= 0.0)
    assert r["accepted"] + r["rejected"] == r["iterations"] == len(r["trace"])
    assert abs(S.cost()["cost"] - r["cost_final"]) <= 1e-12 * r["cost_final"]
    r2 = S.optimize(dx_tol=1e-4)
    assert r2["iterations"] == 1 and r2["reason"] == 1
    S.close()


def test_frozen_after_done(c1):
    """A batch longer than the loop needs: the iterations enqueued after the stop change nothing."""
    A = bos.Solver(c1)
    ra = A.optimize(lambda0=0.01, dx_tol=1e-4, check_every=1)
    B = bos.Solver(c1)
    rb = B.optimize(lambda0=0.01, dx_tol=1e-4, check_every=50)
    assert ra["iterations"] == rb["iterations"] and ra["trace"].tobytes() == rb["trace"].tobytes()
    assert ra["lambda_final"] == rb["lambda_final"] and ra["reason"] == rb["reason"] == 1
    assert _same(A.get_state(), B.get_state())
    A.close()
    B.close()


# ---------------------------------------------------------------- 8. neighbours unaffected
def test_step_after_optimize(c1):
    """fp64: the T caches a GN step reads are the state itself and its cos / sin, which the device's
    box-plus and bos_set_state's host code round alike here. (On an fp32 handle the box-plus keeps
    cosf / sinf as the device rounds them, after bos_optimize as after bos_step, and bos_set_state
    writes the host's: equal to an ulp of fp32, not bit for bit.)"""
    A = bos.Solver(c1)
    A.optimize(lambda0=0.01, max_iterations=3, **NOTOL)
    state = A.get_state()
    sa = A.step()
    B = bos.Solver(c1)
    B.set_state(*state)
    sb = B.step()
    assert _same(A.get_state(), B.get_state())
    assert sa["chi2"] == sb["chi2"] and sa["max_abs_dx"] == sb["max_abs_dx"] and sa["solver_info"] == sb["solver_info"] == 0
    assert len(A.last_dx()) == c1.N
    A.close()
    B.close()


@pytest.mark.parametrize("kind", ["dense", "rf"])
def test_unsupported_handles(c1, kind):
    kw = {"dense": dict(solver=bos.BOS_SOLVER_DENSE_CHOL), "rf": dict(solver=bos.BOS_SOLVER_ROCSOLVER_RF)}[kind]
    S = bos.Solver(c1, **kw)
    before = S.get_state()
    with pytest.raises(bos.BosError, match=r"\(-5\).*bos_optimize"):
        S.optimize()
    assert _same(S.get_state(), before)
    Q = to_oracle(c1)   # bos_cost works on any one-GPU handle
    F = R.cost(Q, before[0], before[1], 1.0)[0]
    assert abs(S.cost()["cost"] - F) <= 1e-9 * F
    S.close()


def test_bad_options(c1):
    S = bos.Solver(c1)
    for kw in (dict(max_iterations=0), dict(max_iterations=4097), dict(check_every=0), dict(lambda0=-1.0),
               dict(lambda_min=0.0), dict(lambda_min=1.0, lambda_max=0.5)):
        with pytest.raises(bos.BosError, match=r"\(-1\)"):
            S.optimize(**kw)
    S.close()


# ---------------------------------------------------------------- 9. agrees with the CPU twin
def test_agrees_with_cpu_twin(c1):
    S = bos.Solver(c1)
    g = S.optimize(lambda0=0.01)
    S.close()
    C = bos.CpuGN(c1, threads=4)
    c = C.optimize(lambda0=0.01)
    C.close()
    print(f"gpu {g['iterations']} it reason {g['reason']} cost {g['cost_final']:.12g}; cpu twin {c['iterations']} it reason "
          f"{c['reason']} cost {c['cost_final']:.12g}")
    assert g["reason"] == c["reason"] and g["reason"] in (1, 2)
    assert abs(g["cost_final"] - c["cost_final"]) <= 1e-6 * c["cost_final"]
