"""Solver.edge_covariances() (bos_edge_covariances: J+H build, multifrontal factorization, selected
inverse with the cross blocks' emission, projection kernel) against a dense inverse of the system the
same call linearised (export_system() right after it), against the host twin, against marginals(), and
for non-interference with the GN steps around it. Reference, error measures and bounds:
tests/edge_cov_ref.py."""
import numpy as np
import pytest

import bos
from conftest import C1, MINI
from edge_cov_ref import (EdgeReference, RefinedEdgeReference, check_information_bound, check_reference, check_refined,
                          check_structure)
from helpers import gpu_lower
from marginals_ref import TOL_CAP, check_blocks, sparse_tol
from test_edge_cov_host import edge_case_world

pytestmark = pytest.mark.gpu

SCHUR, SUPERNODAL = bos.BOS_SOLVER_SCHUR, bos.BOS_SOLVER_SUPERNODAL
KEYS = ("bearing_cross", "odom_cross", "bearing_var", "odom_cov", "pose_cov", "landmark_cov")


@pytest.fixture(scope="module")
def c1():
    return bos.load_g2o(C1)


def _same(a, b, keys=KEYS):
    return all(np.array_equal(a[k], b[k]) for k in keys) and a["solver_info"] == b["solver_info"] == 0


def _accuracy(P, S, what):
    out = S.edge_covariances()
    rows, cols, vals, _ = S.export_system()
    pose, lm = S.get_state()
    ref = RefinedEdgeReference(P, gpu_lower(rows, cols, vals, P.N), pose, lm)
    print(f"edge covariances gpu {what}:")
    assert out["solver_info"] == 0
    check_reference(ref, out, TOL_CAP)
    check_refined(ref, out, what)          # within 8 x the fp64 references' own error of Sigma*
    check_blocks(P, out["pose_cov"], out["landmark_cov"])
    check_structure(P, out)
    return out, vals


@pytest.mark.parametrize("plan", ["schur", "supernodal", "schur_leaf40"])
def test_accuracy_fp64(c1, plan):
    """The three plans: cross blocks out of folded landmarks' S_RJ under wave fronts (and the larger
    fronts of the default plan's top, whose S_RJ stays in the workspace), nested dissection without
    folds, and 40-pose leaves (pairs inside one supernode of more than 64 rows)."""
    kw = {"schur": dict(solver=SCHUR), "supernodal": dict(solver=SUPERNODAL),
          "schur_leaf40": dict(solver=SCHUR, schur_leaf=40)}[plan]
    S = bos.Solver(c1, **kw)
    _accuracy(c1, S, plan)
    S.close()


def test_accuracy_fp32(c1):
    """fp32 J+H, fp64 factor; J of the projection from the fp64 master state: against its own exported system."""
    S = bos.Solver(c1, precision=bos.BOS_FP32)
    _accuracy(c1, S, "fp32")
    S.close()


def test_accuracy_after_steps(c1):
    """At the estimate of 10 GN iterations, the stream still busy with the last step when asked."""
    S = bos.Solver(c1)
    S.step_n(10)
    _accuracy(c1, S, "after 10 steps")
    S.close()


@pytest.mark.parametrize("solver", [SCHUR, SUPERNODAL])
def test_edge_case_world(c1, solver):
    """Duplicates, a reversed duplicate, self-loops, distant loop closures, bearings from the fixed pose."""
    P = edge_case_world(c1)
    S = bos.Solver(P, solver=solver)
    _accuracy(P, S, f"edge cases solver {solver}")
    S.close()


@pytest.mark.parametrize("solver", [SCHUR, SUPERNODAL])
def test_mini_dataset(solver):
    """n = 18: the smallest tree, a supernode whose parent is a root."""
    P = bos.load_g2o(MINI)
    S = bos.Solver(P, solver=solver)
    _accuracy(P, S, f"mini solver {solver}")
    S.close()


@pytest.mark.parametrize("which", ["c1", "c2"])
def test_gpu_matches_host(c1, which):
    """The host twin on the GPU's own exported values gives the GPU's results. Config 2 (synthetic
    1000 / 2000 / 20) has its fronts of 65-128 rows (the MFMA class) in the default plan; its bound
    comes from a sparse estimate of kappa_1 and the host's blocks scale the errors as the reference's
    do in edge_cov_ref.py (cross entries within tol, projected ones within 2 tol)."""
    P = c1 if which == "c1" else bos.synthetic(1000, 2000, 20)
    S = bos.Solver(P)
    out = S.edge_covariances()
    rows, cols, vals, _ = S.export_system()
    S.close()
    assert out["solver_info"] == 0
    host = bos.plan_mf_edge_covariances(P, vals, solver=SCHUR)
    tol, kappa = sparse_tol(P, gpu_lower(rows, cols, vals, P.N))
    # an EdgeReference-shaped scale from the host's diagonal blocks: sd_i per dof, zero on the fixed pose
    sd = np.concatenate([np.sqrt(np.diagonal(host["pose_cov"], axis1=1, axis2=2)).ravel(),
                         np.sqrt(np.diagonal(host["landmark_cov"], axis1=1, axis2=2)).ravel()])
    ref = _host_reference(P, host, sd)
    e_blocks = max(float((np.abs(out[k] - host[k]) / np.maximum(s, 1e-300)).max())
                   for k, s in (("pose_cov", ref.pose_scale), ("landmark_cov", ref.lm_scale)))
    ec = ref.cross_error(out["bearing_cross"], out["odom_cross"])
    ep = ref.projected_error(out["bearing_var"], out["odom_cov"])
    print(f"edge covariances gpu vs host {which}: kappa_1 {kappa:.3g} tol {tol:.3g} blocks {e_blocks:.3g} "
          f"cross {ec:.3g} projected {ep:.3g}")
    check_blocks(P, out["pose_cov"], out["landmark_cov"])
    check_structure(P, out)
    bound = min(tol, TOL_CAP)
    assert e_blocks <= bound and ec <= bound and ep <= 2 * bound
    if which == "c2":
        check_information_bound(P, out)


def _host_reference(P, host, sd):
    """The host twin's results in the shape of an EdgeReference (values and scales), so that its error
    measures apply: J from edge_cov_ref's restatement at P's state."""
    from edge_cov_ref import bearing_jacobians, odometry_jacobians
    ref = EdgeReference.__new__(EdgeReference)
    three, two = np.arange(3), np.arange(2)
    bp = 3 * P.b_pose.astype(np.int64)[:, None] + three
    bl = 3 * P.NP + 2 * P.b_lm.astype(np.int64)[:, None] + two
    oa = 3 * P.o_src.astype(np.int64)[:, None] + three
    ob = 3 * P.o_dst.astype(np.int64)[:, None] + three
    for k in ("bearing_cross", "odom_cross", "bearing_var", "odom_cov"):
        setattr(ref, k, host[k])
    ref.bearing_cross_scale = sd[bp][:, :, None] * sd[bl][:, None, :]
    ref.odom_cross_scale = sd[oa][:, :, None] * sd[ob][:, None, :]
    bi, oi = np.concatenate([bp, bl], axis=1), np.concatenate([oa, ob], axis=1)
    Jb = bearing_jacobians(P.pose_xyt[P.b_pose], P.lm_xy[P.b_lm])
    Jo = odometry_jacobians(P.pose_xyt[P.o_src], P.pose_xyt[P.o_dst])
    ref.bearing_var_scale = (np.abs(Jb) * sd[bi]).sum(axis=1) ** 2
    so = (np.abs(Jo) * sd[oi][:, None, :]).sum(axis=2)
    ref.odom_cov_scale = so[:, :, None] * so[:, None, :]
    sp_, sl_ = sd[:3 * P.NP].reshape(-1, 3), sd[3 * P.NP:].reshape(-1, 2)
    ref.pose_scale = sp_[:, :, None] * sp_[:, None, :]
    ref.pose_scale[P.fixed] = 1.0
    ref.lm_scale = sl_[:, :, None] * sl_[:, None, :]
    return ref


def test_deterministic(c1):
    S = bos.Solver(c1)
    a = S.edge_covariances()
    b = S.edge_covariances()
    S.close()
    assert _same(a, b)


@pytest.mark.parametrize("first", ["edge_covariances", "marginals"])
def test_blocks_equal_marginals(c1, first):
    """pose_cov / landmark_cov are bit for bit marginals()' on the same handle, in either call order."""
    S = bos.Solver(c1)
    if first == "marginals":
        pose, lm, info = S.marginals()
        out = S.edge_covariances()
    else:
        out = S.edge_covariances()
        pose, lm, info = S.marginals()
    S.close()
    assert info == out["solver_info"] == 0
    assert np.array_equal(out["pose_cov"], pose) and np.array_equal(out["landmark_cov"], lm)


@pytest.mark.parametrize("precision", [bos.BOS_FP64, bos.BOS_FP32])
def test_steps_do_not_see_the_call(c1, precision):
    """The state is bit-identical across edge_covariances(); step, edge_covariances, step ends where
    step, step does."""
    A = bos.Solver(c1, precision=precision)
    B = bos.Solver(c1, precision=precision)
    A.step()
    B.step()
    before = A.get_state()
    A.edge_covariances()
    after = A.get_state()
    assert np.array_equal(before[0], after[0]) and np.array_equal(before[1], after[1])
    sa = A.step()
    sb = B.step()
    pa, la = A.get_state()
    pb, lb = B.get_state()
    A.close()
    B.close()
    assert np.array_equal(pa, pb) and np.array_equal(la, lb)
    assert sa["chi2"] == sb["chi2"] and sa["solver_info"] == sb["solver_info"] == 0


def test_null_outputs(c1):
    """Every combination of the three output groups returns the same bits for what it returns."""
    S = bos.Solver(c1)
    full = S.edge_covariances()
    groups = {"cross": KEYS[0:2], "projected": KEYS[2:4], "blocks": KEYS[4:6]}
    for mask in range(7):
        kw = {g: bool(mask >> i & 1) for i, g in enumerate(groups)}
        out = S.edge_covariances(**kw)
        assert out["solver_info"] == 0
        for g, keys in groups.items():
            for k in keys:
                assert (np.array_equal(out[k], full[k]) if kw[g] else out[k] is None), (kw, k)
    S.close()


@pytest.mark.parametrize("kind", ["dense", "rf", "communicator"])
def test_unsupported_handles(c1, kind):
    kw = {"dense": dict(solver=bos.BOS_SOLVER_DENSE_CHOL), "rf": dict(solver=bos.BOS_SOLVER_ROCSOLVER_RF),
          "communicator": dict(solver=SCHUR, rank=0, world_size=1, nccl_id=bos.nccl_unique_id())}[kind]
    S = bos.Solver(c1, **kw)
    with pytest.raises(bos.BosError, match=r"\(-5\).*bos_edge_covariances"):
        S.edge_covariances()
    S.close()
