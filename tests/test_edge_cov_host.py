"""Edge covariances on the host (bos_plan_mf_edge_covariances: HostMf::selected_inverse with the plan's
cross records, then the projection of csrc/host/edge_cov.hpp) against a dense inverse of the oracle's
H_nf. Reference, error measures and bounds: tests/edge_cov_ref.py."""
import numpy as np
import pytest

import bos
import oracle as O
from conftest import C1, MINI
from edge_cov_ref import EdgeReference, check_information_bound, check_reference, check_structure
from helpers import oracle_lower_nf, to_oracle
from marginals_ref import TOL_CAP, check_blocks

SCHUR, SUPERNODAL = bos.BOS_SOLVER_SCHUR, bos.BOS_SOLVER_SUPERNODAL


def edge_case_world(P, seed=11):
    """P plus the edges the headline datasets lack: duplicated bearings, a reversed duplicate of an
    odometry edge (and a same-orientation duplicate), odometry self-loops (one on the fixed pose), loop
    closures between distant poses (one of them from the fixed pose) and bearings taken from the fixed
    pose. Measurements are the current estimate's predictions plus noise."""
    rng = np.random.default_rng(seed)
    Q = to_oracle(P)
    fx = P.fixed
    free = np.array([p for p in range(P.NP) if p != fx])
    kb = rng.choice(len(P.b_z), 40, replace=False)
    lf = rng.choice(P.NL, 5, replace=False)
    b_pose = np.concatenate([P.b_pose, P.b_pose[kb], np.full(len(lf), fx)])
    b_lm = np.concatenate([P.b_lm, P.b_lm[kb], lf])
    zf = [O.predict_bearing(Q.pose_xyt[fx], Q.lm_xy[l]) for l in lf]
    b_z = np.concatenate([P.b_z, P.b_z[kb] + rng.normal(0, 0.01, len(kb)), np.array(zf) + rng.normal(0, 0.01, len(lf))])
    ko = rng.choice(len(P.o_z), 6, replace=False)
    far_s = rng.choice(free[free < P.NP - 60], 5, replace=False)
    loops = np.concatenate([rng.choice(free, 3, replace=False), [fx]])
    src = np.concatenate([P.o_dst[ko[:3]], P.o_src[ko[3:]], far_s, [fx], loops])
    dst = np.concatenate([P.o_src[ko[:3]], P.o_dst[ko[3:]], far_s + 60, [(fx + P.NP // 2) % P.NP], loops])
    z = np.array([O.predict_odometry(Q.pose_xyt[s], Q.pose_xyt[d]) for s, d in zip(src, dst)]) + rng.normal(0, 0.03, (len(src), 3))
    om = P.o_omega[rng.choice(len(P.o_z), len(src))]
    return bos.Problem(P.pose_xyt, P.lm_xy, b_pose, b_lm, b_z, np.concatenate([P.o_src, src]), np.concatenate([P.o_dst, dst]),
                       np.concatenate([P.o_z, z]), np.concatenate([P.o_omega, om]), fx, b_omega=P.b_omega,
                       pose_ids=P.pose_ids, lm_ids=P.lm_ids)


_cache = {}


def _case(which, damping):
    """Problem, the oracle's lower H_nf and its dense reference: computed once per (dataset, damping)."""
    key = (which, damping)
    if key not in _cache:
        P = bos.load_g2o(MINI if which == "mini" else C1)
        if which == "edge_cases":
            P = edge_case_world(P)
        Q = to_oracle(P)
        Hl = oracle_lower_nf(Q, O.linearize(Q, damping=damping)).tocsr()
        _cache[key] = (P, Hl, EdgeReference(P, Hl))
    return _cache[key]


def _run(which, damping, solver, schur_leaf=0):
    P, Hl, ref = _case(which, damping)
    info = bos.plan_inspect(P, 0, 1, entries=True, solver=solver, schur_leaf=schur_leaf)
    vals = np.asarray(Hl[info["rows"], info["cols"]]).ravel()
    out = bos.plan_mf_edge_covariances(P, vals, solver=solver, schur_leaf=schur_leaf)
    print(f"edge covariances host {which} damping {damping} solver {solver} leaf {schur_leaf} "
          f"max front {info['mf_max_front']}:")
    check_reference(ref, out, TOL_CAP)
    check_blocks(P, out["pose_cov"], out["landmark_cov"])
    check_structure(P, out)
    pose, lm = bos.plan_mf_marginals(P, vals, solver=solver, schur_leaf=schur_leaf)
    assert np.array_equal(out["pose_cov"], pose) and np.array_equal(out["landmark_cov"], lm)
    return P, out, info


@pytest.mark.parametrize("damping", [0.01, 1.0])
def test_schur_plan(damping):
    """The default Schur plan: a bearing's cross block is a piece of its folded landmark's S_RJ."""
    _run("c1", damping, SCHUR)


def test_supernodal_plan():
    """Nested dissection of poses and landmarks together: pairs inside one supernode (S_JJ) as well."""
    _run("c1", 0.01, SUPERNODAL)


def test_schur_plan_with_large_fronts():
    """40-pose leaves: fronts of more than 64 rows, most pose pairs inside one supernode."""
    _, _, info = _run("c1", 0.01, SCHUR, schur_leaf=40)
    assert info["mf_max_front"] > 64


@pytest.mark.parametrize("solver", [SCHUR, SUPERNODAL])
def test_mini_dataset(solver):
    """n = 18: the smallest tree, a supernode whose parent is a root."""
    _run("mini", 0.01, solver)


@pytest.mark.parametrize("solver", [SCHUR, SUPERNODAL])
def test_edge_case_world(solver):
    """Duplicates, a reversed duplicate, self-loops, distant loop closures and bearings from the fixed
    pose: the reference bounds and the exact zero / transpose / equality rules."""
    P, out, _ = _run("edge_cases", 0.01, solver)
    fx = P.fixed
    assert (P.b_pose == fx).sum() >= 5 and (P.o_src == P.o_dst).sum() == 4
    assert ((P.o_src == fx) ^ (P.o_dst == fx)).sum() >= 1
    pairs = set(zip(P.o_src.tolist(), P.o_dst.tolist()))
    assert any((b, a) in pairs for a, b in pairs if a != b)            # a reversed duplicate exists
    assert len(pairs) < len(P.o_src)                                   # and a same-orientation one
    assert len(set(zip(P.b_pose.tolist(), P.b_lm.tolist()))) < len(P.b_z)


@pytest.mark.parametrize("which", ["c1", "edge_cases"])
def test_information_bound(which):
    """omega bearing_var < 1 and eig(Omega^1/2 odom_cov Omega^1/2) < 1: no reference involved."""
    P, Hl, _ = _case(which, 0.01)
    info = bos.plan_inspect(P, 0, 1, entries=True, solver=SCHUR)
    vals = np.asarray(Hl[info["rows"], info["cols"]]).ravel()
    check_information_bound(P, bos.plan_mf_edge_covariances(P, vals, solver=SCHUR))
