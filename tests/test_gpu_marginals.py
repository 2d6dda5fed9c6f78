"""Solver.marginals() (bos_marginals: J+H build, multifrontal factorization, selected inverse on the
device) against a dense inverse of the system the same call linearised (export_system() right after
it), against the host recursion, and for non-interference with the GN steps around it. Reference,
error measure, the derived bound tol = n eps kappa_1(H_s) and the refined criterion (Sigma* refined in
np.longdouble, the bound 8 e_ref measured from two fp64 inverses): tests/marginals_ref.py."""
import types

import numpy as np
import pytest

import bos
from conftest import C1
from helpers import gpu_lower
from marginals_ref import TOL_CAP, RefinedReference, check_blocks, scaled_diff, sparse_tol

pytestmark = pytest.mark.gpu

SCHUR, SUPERNODAL = bos.BOS_SOLVER_SCHUR, bos.BOS_SOLVER_SUPERNODAL


@pytest.fixture(scope="module")
def c1():
    return bos.load_g2o(C1)


def _accuracy(P, S, what):
    pose, lm, info = S.marginals()
    rows, cols, vals, _ = S.export_system()
    ref = RefinedReference(P, gpu_lower(rows, cols, vals, P.N))
    e = ref.error(pose, lm)
    print(f"marginals gpu {what}: n {ref.n} kappa_1 {ref.kappa:.3g} tol {ref.tol:.3g} err {e:.3g}")
    assert info == 0
    assert ref.tol <= TOL_CAP
    assert e <= ref.tol
    ref.check_refined(pose, lm, what)      # within 8 x the fp64 references' own error of Sigma*
    check_blocks(P, pose, lm)
    return pose, lm, vals, ref


@pytest.mark.parametrize("plan", ["schur", "supernodal", "schur_leaf40"])
def test_accuracy_fp64(c1, plan):
    """The three plans: folded landmarks under wave fronts (and the larger fronts of the default
    plan's top), nested dissection without folds, and 40-pose leaves (folds into fronts of more than
    64 rows)."""
    kw = {"schur": dict(solver=SCHUR), "supernodal": dict(solver=SUPERNODAL),
          "schur_leaf40": dict(solver=SCHUR, schur_leaf=40)}[plan]
    S = bos.Solver(c1, **kw)
    _accuracy(c1, S, plan)
    S.close()


def test_accuracy_fp32(c1):
    """fp32 J+H (the folds read the fp32 block array), fp64 factor: against its own exported system."""
    S = bos.Solver(c1, precision=bos.BOS_FP32)
    _accuracy(c1, S, "fp32")
    S.close()


def test_accuracy_after_steps(c1):
    """At the estimate of 10 GN iterations, the stream still busy with the last step when asked."""
    S = bos.Solver(c1)
    S.step_n(10)
    _accuracy(c1, S, "after 10 steps")
    S.close()


@pytest.mark.parametrize("which", ["c1", "c2"])
def test_gpu_matches_host(c1, which):
    """The host recursion on the GPU's own exported values gives the GPU's blocks. Config 2
    (synthetic 1000 / 2000 / 20) has its fronts of 65-128 rows in the default plan; its bound comes
    from a sparse estimate of kappa_1 (no dense inverse of n = 6 997) and the host's blocks scale
    the error."""
    P = c1 if which == "c1" else bos.synthetic(1000, 2000, 20)
    S = bos.Solver(P)
    pose, lm, info = S.marginals()
    rows, cols, vals, _ = S.export_system()
    S.close()
    assert info == 0
    hp, hl = bos.plan_mf_marginals(P, vals, solver=SCHUR)
    tol, kappa = sparse_tol(P, gpu_lower(rows, cols, vals, P.N))
    scale = types.SimpleNamespace(pose=hp.copy(), lm=hl, fixed=P.fixed)
    scale.pose[P.fixed] = np.eye(3)
    e = scaled_diff(pose, lm, hp, hl, scale)
    print(f"marginals gpu vs host {which}: kappa_1 {kappa:.3g} tol {tol:.3g} diff {e:.3g}")
    check_blocks(P, pose, lm)
    assert e <= min(tol, TOL_CAP)


def test_deterministic(c1):
    S = bos.Solver(c1)
    a = S.marginals()
    b = S.marginals()
    S.close()
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and a[2] == b[2] == 0


@pytest.mark.parametrize("precision", [bos.BOS_FP64, bos.BOS_FP32])
def test_steps_do_not_see_the_call(c1, precision):
    """The state is bit-identical across marginals(); step, marginals, step ends where step, step does."""
    A = bos.Solver(c1, precision=precision)
    B = bos.Solver(c1, precision=precision)
    A.step()
    B.step()
    before = A.get_state()
    A.marginals()
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
    S = bos.Solver(c1)
    pose, lm, _ = S.marginals()
    p2, none, i2 = S.marginals(landmarks=False)
    none2, l3, i3 = S.marginals(poses=False)
    S.close()
    assert none is None and none2 is None and i2 == i3 == 0
    assert np.array_equal(pose, p2) and np.array_equal(lm, l3)


@pytest.mark.parametrize("kind", ["dense", "rf", "communicator"])
def test_unsupported_handles(c1, kind):
    kw = {"dense": dict(solver=bos.BOS_SOLVER_DENSE_CHOL), "rf": dict(solver=bos.BOS_SOLVER_ROCSOLVER_RF),
          "communicator": dict(solver=SCHUR, rank=0, world_size=1, nccl_id=bos.nccl_unique_id())}[kind]
    S = bos.Solver(c1, **kw)
    with pytest.raises(bos.BosError, match=r"\(-5\).*bos_marginals"):
        S.marginals()
    S.close()
