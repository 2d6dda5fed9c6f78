"""Solver.joint_compatibility() (bos_joint_compatibility: J+H build, multifrontal factorization, the pair call's
path solve and products, then one wavefront per hypothesis: S in LDS, its LDL^T and the prefix NIS) against a
dense inverse of the system the same call linearised (export_system() right after it), against
pair_covariances() and associate_bearings() on the same handle, against the host twin, and for
non-interference with the GN steps around it. Reference, hypotheses and bounds: tests/joint_ref.py."""
import numpy as np
import pytest

import bos
from associate_ref import AssocReference
from conftest import C1, MINI
from edge_cov_ref import bearing_jacobians
from helpers import EPS, gpu_lower
from joint_ref import JointReference, check_exact_rules, check_recurrence, make_hypotheses, s_offdiag
from marginals_ref import TOL_CAP, DenseInverses, sparse_tol
from test_edge_cov_host import edge_case_world

pytestmark = pytest.mark.gpu

SCHUR, SUPERNODAL = bos.BOS_SOLVER_SCHUR, bos.BOS_SOLVER_SUPERNODAL


@pytest.fixture(scope="module")
def c1():
    return bos.load_g2o(C1)


_dense = {}


def _dense_of(P, Hl, vals):
    """The dense inverses of one exported system, shared by the handles that export the same bits."""
    key = (P.N, vals.tobytes())
    if key not in _dense:
        _dense[key] = DenseInverses(P, Hl)
    return _dense[key]


def _call(S, start, pose, landmark, z, omega, batch=0):
    S.debug_set_joint_batch(batch)
    out = S.joint_compatibility((start, pose, landmark), z, omega, cov=True)
    S.debug_set_joint_batch(0)
    assert out["solver_info"] == 0
    return out


def _accuracy(P, S, what, solver=SCHUR, leaf=0):
    state = S.get_state()
    H = make_hypotheses(P, state, solver, leaf)
    out = _call(S, *H.arrays())
    rows, cols, vals, _ = S.export_system()
    Hl = gpu_lower(rows, cols, vals, P.N)
    ref = JointReference(P, Hl, *H.arrays(), pose_xyt=state[0], lm_xy=state[1], dense=_dense_of(P, Hl, vals))
    ref.check(out, f"gpu {what}")
    check_recurrence(out)
    return H, out


PLAN_KW = {"schur": dict(solver=SCHUR), "supernodal": dict(solver=SUPERNODAL), "schur_leaf40": dict(solver=SCHUR, schur_leaf=40)}


@pytest.mark.parametrize("plan", ["schur", "supernodal", "schur_leaf40"])
def test_accuracy_fp64(c1, plan):
    """C1's three plans, with fronts over 64 rows."""
    kw = PLAN_KW[plan]
    fronts = bos.plan_mf_fronts(c1, **kw)
    assert (fronts[:, 0] + fronts[:, 1]).max() > 64
    S = bos.Solver(c1, **kw)
    _accuracy(c1, S, plan, kw["solver"], kw.get("schur_leaf", 0))
    S.close()


@pytest.mark.parametrize("solver", [SCHUR, SUPERNODAL])
def test_mini_dataset(solver):
    P = bos.load_g2o(MINI)
    S = bos.Solver(P, solver=solver)
    _accuracy(P, S, f"mini solver {solver}", solver)
    S.close()


def test_register_class_alone():
    """bos.synthetic(60, 120, 6): every front has at most 64 rows."""
    P = bos.synthetic(60, 120, 6)
    fronts = bos.plan_mf_fronts(P, solver=SCHUR)
    assert (fronts[:, 0] + fronts[:, 1]).max() <= 64
    S = bos.Solver(P, solver=SCHUR)
    _accuracy(P, S, "synthetic 60/120/6", SCHUR)
    S.close()


def test_edge_case_world(c1):
    P = edge_case_world(c1)
    S = bos.Solver(P, solver=SCHUR)
    _accuracy(P, S, "edge cases", SCHUR)
    S.close()


def test_accuracy_fp32(c1):
    """fp32 J+H, fp64 factor; e and J from the fp64 master state: against its own exported system."""
    S = bos.Solver(c1, precision=bos.BOS_FP32)
    _accuracy(c1, S, "fp32")
    S.close()


def test_accuracy_after_steps(c1):
    """At the estimate of 10 GN iterations, the stream still busy with the last step when asked."""
    S = bos.Solver(c1)
    S.step_n(10)
    _accuracy(c1, S, "after 10 steps")
    S.close()


def test_against_pair_covariances_and_association(c1):
    """S_ii - 1 / omega_i is pair_covariances()' projected[0] of (pose_i, NP + landmark_i), bit for bit; an
    off-diagonal entry is s_offdiag of pair_covariances()' blocks and NumPy's Jacobians within 64 eps s_i s_j
    (the device's J is not returned; its entries differ from NumPy's by a few ulp, 25 products of |J| sd sd |J|
    sum to at most s_i s_j); an m = 1 hypothesis agrees with associate_bearings()' nis_all entry within
    associate_ref's bound."""
    P = c1
    S = bos.Solver(P)
    state = S.get_state()
    H = make_hypotheses(P, state, SCHUR)
    out = _call(S, *H.arrays())
    worst = 0.0
    for name in ("single", "three_poses", "m32_one_pose", "m32_random", "fixed_pose", "shared_landmark", "pairing_twice"):
        h = H.index[name]
        p, l, _, om = H.one(h)
        Sh = out["innovation_cov"][h]
        pc = S.pair_covariances(p, P.NP + l)
        assert np.array_equal(np.diag(Sh), pc["projected"][:, 0] + 1.0 / om), name
        J = bearing_jacobians(state[0][p], state[1][l])
        sd = np.sqrt(np.concatenate([np.diagonal(pc["cov_a"].reshape(-1, 3, 3), axis1=1, axis2=2),
                                     np.diagonal(pc["cov_b"][:, :4].reshape(-1, 2, 2), axis1=1, axis2=2)], axis=1))   # [m, 5]
        s = (np.abs(J) * sd).sum(axis=1)
        m = min(len(p), 8)
        nodes = np.stack([p, P.NP + l], axis=1)
        qa, qb, where = [], [], []
        for i in range(1, m):
            for j in range(i):
                for bi, u in enumerate(nodes[i]):
                    for bj, v in enumerate(nodes[j]):
                        qa.append(min(u, v)); qb.append(max(u, v)); where.append((i, j, bi, bj, u <= v, u == v))
        blocks = S.pair_covariances(qa, qb) if qa else None
        C = {}
        for q, (i, j, bi, bj, straight, same) in enumerate(where):
            da, db = (3 if qa[q] < P.NP else 2), (3 if qb[q] < P.NP else 2)
            blk = (blocks["cov_a"] if same else blocks["cross"])[q, :da * db].reshape(da, db)
            blk = blk if straight else blk.T
            C.setdefault((i, j), np.zeros((5, 5)))[3 * bi:3 * bi + blk.shape[0], 3 * bj:3 * bj + blk.shape[1]] = blk
        for (i, j), Cij in C.items():
            d = abs(Sh[i, j] - s_offdiag(Cij, J[i], J[j]))
            worst = max(worst, d / (s[i] * s[j]))
            assert d <= 64 * EPS * s[i] * s[j], (name, i, j)
    print(f"joint vs pair_covariances blocks: worst off-diagonal difference {worst:.3g} of s_i s_j (bound {64 * EPS:.3g})")
    h = H.index["single"]
    p, l, z, om = H.one(h)
    assoc = S.associate_bearings(p, z, om, nis_all=True)
    rows, cols, vals, _ = S.export_system()
    Hl = gpu_lower(rows, cols, vals, P.N)
    ar = AssocReference(P, Hl, p, z, om, state[0], state[1], dense=_dense_of(P, Hl, vals))
    d = abs(out["joint_nis"][h] - assoc["nis_all"][0, l[0]])
    print(f"joint m = 1 vs association: |difference| {d:.3g} bound {ar.bound[0, l[0]]:.3g}")
    assert d <= ar.bound[0, l[0]]
    S.close()


@pytest.mark.parametrize("which", ["c1", "edge_cases"])
def test_exact_rules(c1, which):
    """Two calls, prefixes, the repeat, order, company and one hypothesis per batch: identical bits."""
    P = c1 if which == "c1" else edge_case_world(c1)
    S = bos.Solver(P)
    H = make_hypotheses(P, S.get_state(), SCHUR)
    out = check_exact_rules(H, lambda *a, batch=0: _call(S, *a, batch=batch))
    assert out["joint_nis"][H.index["empty"]] == 0.0
    S.close()


def test_null_outputs_and_forms(c1):
    """A call without cov returns the same bits for the rest; the list form is the flat form."""
    S = bos.Solver(c1)
    H = make_hypotheses(c1, S.get_state(), SCHUR)
    full = _call(S, *H.arrays())
    start, p, l, z, om = H.arrays()
    lean = S.joint_compatibility((start, p, l), z, om)
    assert lean["innovation_cov"] is None
    listed = S.joint_compatibility([H.one(h) for h in range(len(H))], cov=True)
    for k in ("prefix_nis", "joint_nis", "innovation"):
        assert np.array_equal(lean[k], full[k]) and np.array_equal(listed[k], full[k]), k
    assert all(np.array_equal(x, y) for x, y in zip(listed["innovation_cov"], full["innovation_cov"]))
    ones = S.joint_compatibility((start, p, l), z, np.ones(len(z)))
    none = S.joint_compatibility((start, p, l), z)
    assert np.array_equal(ones["prefix_nis"], none["prefix_nis"])
    t = S.joint_compatibility_timing()
    assert t["joint_bytes"] > 0 and t["factor_ms"] > 0 and t["path_ms"] > 0 and t["nis_ms"] > 0
    S.close()


def test_gpu_matches_host(c1):
    """The host twin on the GPU's own exported values: S within min(sparse tol, 1e-6) (2 x, as a projected entry)
    in the S measure, s_i from the host's own blocks; e within 64 eps; every prefix NIS within joint_ref's bound
    evaluated with that tolerance."""
    P = c1
    S = bos.Solver(P)
    H = make_hypotheses(P, S.get_state(), SCHUR)
    out = _call(S, *H.arrays())
    rows, cols, vals, _ = S.export_system()
    S.close()
    start, p, l, z, om = H.arrays()
    host = bos.plan_mf_joint_compatibility(P, vals, (start, p, l), z, om, solver=SCHUR)
    tol, kappa = sparse_tol(P, gpu_lower(rows, cols, vals, P.N))
    bound = min(tol, TOL_CAP)
    pc = bos.plan_mf_pair_covariances(P, vals, p, P.NP + l, solver=SCHUR)
    sd = np.sqrt(np.concatenate([np.diagonal(pc["cov_a"].reshape(-1, 3, 3), axis1=1, axis2=2),
                                 np.diagonal(pc["cov_b"][:, :4].reshape(-1, 2, 2), axis1=1, axis2=2)], axis=1))
    s_all = (np.abs(bearing_jacobians(P.pose_xyt[p], P.lm_xy[l])) * sd).sum(axis=1)
    eS = eN = 0.0
    for h in range(len(H)):
        q = slice(start[h], start[h + 1])
        if start[h + 1] == start[h]:
            continue
        s = s_all[q]
        Sg, Sh, e = out["innovation_cov"][h], host["innovation_cov"][h], host["innovation"][q]
        eS = max(eS, float((np.abs(Sg - Sh) / np.outer(s, s)).max()))
        assert np.all(np.abs(out["innovation"][q] - e) <= 64 * EPS)
        for k in range(len(e)):
            x = np.linalg.solve(Sh[:k + 1, :k + 1], e[:k + 1])
            b = 2 * bound * (np.abs(x) * s[:k + 1]).sum() ** 2 + 64 * EPS * (k + 1) * np.linalg.cond(Sh[:k + 1, :k + 1]) * host["prefix_nis"][q][k]
            eN = max(eN, abs(out["prefix_nis"][q][k] - host["prefix_nis"][q][k]) / b)
    print(f"joint gpu vs host: kappa_1 {kappa:.3g} tol {tol:.3g}: S {eS:.3g}, worst |nis - host| / bound {eN:.3g}")
    assert eS <= 2 * bound and eN <= 1.0


@pytest.mark.parametrize("precision", [bos.BOS_FP64, bos.BOS_FP32])
def test_steps_do_not_see_the_call(c1, precision):
    """The state is bit-identical across joint_compatibility(); step, call, step ends where step, step does."""
    A = bos.Solver(c1, precision=precision)
    B = bos.Solver(c1, precision=precision)
    A.step()
    B.step()
    before = A.get_state()
    H = make_hypotheses(c1, before, SCHUR)
    _call(A, *H.arrays())
    after = A.get_state()
    assert np.array_equal(before[0], after[0]) and np.array_equal(before[1], after[1])
    with pytest.raises(bos.BosError, match=r"\(-1\)"):
        A.last_dx()                                              # as after bos_marginals
    sa = A.step()
    sb = B.step()
    pa, la = A.get_state()
    pb, lb = B.get_state()
    A.close()
    B.close()
    assert np.array_equal(pa, pb) and np.array_equal(la, lb)
    assert sa["chi2"] == sb["chi2"] and sa["solver_info"] == sb["solver_info"] == 0


def test_empty_call_and_bad_arguments(c1):
    S = bos.Solver(c1)
    S.step()
    dx = S.last_dx()
    out = S.joint_compatibility([])
    assert len(out["joint_nis"]) == 0 and out["solver_info"] == 0
    assert np.array_equal(S.last_dx(), dx)                       # n_hyp = 0 touched nothing
    NP, NL, big = c1.NP, c1.NL, bos.JOINT_MAX_M + 1
    bad = [(([1, 2], [1, 1], [0, 0]), [0.1, 0.1], None), (([0, 2, 1], [1], [0]), [0.1], None),
           (([0, big], [1] * big, [0] * big), [0.1] * big, None),
           (([0, 1], [-1], [0]), [0.1], None), (([0, 1], [NP], [0]), [0.1], None),
           (([0, 1], [1], [-1]), [0.1], None), (([0, 1], [1], [NL]), [0.1], None),
           (([0, 1], [1], [0]), [np.nan], None), (([0, 1], [1], [0]), [np.inf], None),
           (([0, 1], [1], [0]), [0.1], [0.0]), (([0, 1], [1], [0]), [0.1], [-2.0]), (([0, 1], [1], [0]), [0.1], [np.nan]),
           (([0, 1], [1], [0]), [0.1], [np.inf])]
    for hyp, z, om in bad:
        with pytest.raises(bos.BosError, match=r"\(-1\)"):
            S.joint_compatibility(hyp, z, om)
    assert np.array_equal(S.last_dx(), dx)
    S.close()


@pytest.mark.parametrize("kind", ["dense", "rf", "communicator"])
def test_unsupported_handles(c1, kind):
    kw = {"dense": dict(solver=bos.BOS_SOLVER_DENSE_CHOL), "rf": dict(solver=bos.BOS_SOLVER_ROCSOLVER_RF),
          "communicator": dict(solver=SCHUR, rank=0, world_size=1, nccl_id=bos.nccl_unique_id())}[kind]
    S = bos.Solver(c1, **kw)
    with pytest.raises(bos.BosError, match=r"\(-5\).*bos_joint_compatibility"):
        S.joint_compatibility([([1], [0], [0.1])])
    S.close()
