"""Marginal covariances on the host (bos_plan_mf_marginals: HostMf::selected_inverse over the plan's
assembly tree) against a dense inverse of the oracle's H_nf. Reference, error measure and the derived
bound tol = n eps kappa_1(H_s): tests/marginals_ref.py."""
import numpy as np
import pytest

import bos
import oracle as O
from conftest import C1, MINI
from helpers import oracle_lower_nf, to_oracle
from marginals_ref import TOL_CAP, Reference, check_blocks

_cache = {}


def _case(which, damping):
    """Problem, the oracle's lower H_nf and its dense reference: computed once per (dataset, damping)."""
    key = (which, damping)
    if key not in _cache:
        P = bos.load_g2o(C1 if which == "c1" else MINI)
        Q = to_oracle(P)
        Hl = oracle_lower_nf(Q, O.linearize(Q, damping=damping)).tocsr()
        _cache[key] = (P, Hl, Reference(P, Hl))
    return _cache[key]


def _run(which, damping, solver, schur_leaf=0):
    P, Hl, ref = _case(which, damping)
    info = bos.plan_inspect(P, 0, 1, entries=True, solver=solver, schur_leaf=schur_leaf)
    vals = np.asarray(Hl[info["rows"], info["cols"]]).ravel()
    pose, lm = bos.plan_mf_marginals(P, vals, solver=solver, schur_leaf=schur_leaf)
    e = ref.error(pose, lm)
    print(f"marginals host {which} damping {damping} solver {solver} leaf {schur_leaf}: n {ref.n} "
          f"kappa_1 {ref.kappa:.3g} tol {ref.tol:.3g} err {e:.3g} max front {info['mf_max_front']}")
    assert ref.tol <= TOL_CAP
    assert e <= ref.tol
    check_blocks(P, pose, lm)
    return info


@pytest.mark.parametrize("damping", [0.01, 1.0])
def test_schur_plan(damping):
    """The default Schur plan: every landmark a folded 2-column supernode below a pose front."""
    _run("c1", damping, bos.BOS_SOLVER_SCHUR)


def test_supernodal_plan():
    """Nested dissection of poses and landmarks together: no folds, larger fronts."""
    _run("c1", 0.01, bos.BOS_SOLVER_SUPERNODAL)


def test_schur_plan_with_large_fronts():
    """40-pose leaves: fronts of more than 64 rows (the classes above the one-wavefront fronts)."""
    info = _run("c1", 0.01, bos.BOS_SOLVER_SCHUR, schur_leaf=40)
    assert info["mf_max_front"] > 64


@pytest.mark.parametrize("solver", [bos.BOS_SOLVER_SCHUR, bos.BOS_SOLVER_SUPERNODAL])
def test_mini_dataset(solver):
    """n = 18: the smallest tree, a supernode whose parent is a root."""
    _run("mini", 0.01, solver)
