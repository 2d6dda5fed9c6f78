"""Pair covariances on the host (bos_plan_mf_pair_covariances: one root-path solve per distinct node over
HostMf's factor, the products over the common tail, the projection of csrc/host/pair_cov.hpp) against a
dense inverse of the oracle's H_nf, and bos_plan_pair_paths. Reference, pair sets, error measures and
bounds: tests/pair_cov_ref.py."""
import numpy as np
import pytest

import bos
import oracle as O
from conftest import C1, MINI
from helpers import oracle_lower_nf, to_oracle
from marginals_ref import DenseInverses
from pair_cov_ref import (CLASSES, KEYS, PairReference, check_reference, check_refined, check_rules, dims, node_dofs,
                          pair_set)
from test_edge_cov_host import edge_case_world

SCHUR, SUPERNODAL = bos.BOS_SOLVER_SCHUR, bos.BOS_SOLVER_SUPERNODAL

_cache = {}


def _case(which):
    """Problem, the oracle's lower H_nf (damping 0.01) and its dense inverses: once per world."""
    if which not in _cache:
        P = bos.load_g2o(MINI if which == "mini" else C1)
        if which == "edge_cases":
            P = edge_case_world(P)
        Q = to_oracle(P)
        Hl = oracle_lower_nf(Q, O.linearize(Q, damping=0.01)).tocsr()
        _cache[which] = (P, Hl, DenseInverses(P, Hl))
    return _cache[which]


def _run(which, solver, schur_leaf=0):
    key = (which, solver, schur_leaf)
    if key not in _cache:
        P, Hl, dense = _case(which)
        a, b, classes = pair_set(P, solver, schur_leaf)
        info = bos.plan_inspect(P, 0, 1, entries=True, solver=solver, schur_leaf=schur_leaf)
        vals = np.asarray(Hl[info["rows"], info["cols"]]).ravel()
        out = bos.plan_mf_pair_covariances(P, vals, a, b, solver=solver, schur_leaf=schur_leaf)
        _cache[key] = (P, a, b, classes, out, PairReference(P, Hl, a, b, dense=dense), vals, info)
    return _cache[key]


PLANS = [("mini", SCHUR, 0), ("mini", SUPERNODAL, 0), ("c1", SCHUR, 0), ("c1", SUPERNODAL, 0), ("c1", SCHUR, 40),
         ("edge_cases", SCHUR, 0), ("edge_cases", SUPERNODAL, 0)]


@pytest.mark.parametrize("which,solver,leaf", PLANS)
def test_accuracy(which, solver, leaf):
    """Reference bounds, the refined criterion and the exact rules on 200 random pairs of each kind plus
    the constructed ones."""
    P, a, b, _, out, ref, _, info = _run(which, solver, leaf)
    label = f"host {which} solver {solver} leaf {leaf} max front {info['mf_max_front']}"
    check_reference(ref, out, label)
    check_refined(ref, out, label)
    check_rules(P, a, b, out, ref)


@pytest.mark.parametrize("which,solver,leaf", PLANS)
def test_constructed_classes(which, solver, leaf):
    """plan_pair_paths shows every constructed kind the plan can have, and its columns agree with the
    plan's tree."""
    P, a, b, classes, _, _, _, _ = _run(which, solver, leaf)
    fronts = bos.plan_mf_fronts(P, solver=solver, schur_leaf=leaf)
    print(f"pair classes {which} solver {solver} leaf {leaf}: " + ", ".join(f"{k} {len(classes[k])}" for k in CLASSES))
    always = ("fixed_pose_pose", "fixed_pose_landmark", "self_pair", "duplicate", "reverse")
    tree = ("root_from_two_subtrees", "same_supernode", "ancestor")
    needed = always + (tree if which != "mini" else ()) + (("folded_landmark_unobserved",) if fronts[:, 6].any() and which != "mini" else ())
    for k in needed:
        assert classes[k], k
    paths = bos.plan_pair_paths(P, a, b, solver=solver, schur_leaf=leaf)

    def chain(s):                       # s and its ancestors, and their own dofs
        out = []
        while s >= 0:
            out.append(s)
            s = fronts[s, 3] if fronts[s, 1] > 0 else -1
        return out

    for q in np.concatenate([np.arange(0, len(a), 37), np.concatenate([np.asarray(v, dtype=int) for v in classes.values()])]):
        sa, sb, lca, c, longest = paths[q]
        if a[q] == P.fixed or b[q] == P.fixed:
            assert lca == -2 and c == 0
            assert (sa == -1) == (a[q] == P.fixed) and (sb == -1) == (b[q] == P.fixed)
            continue
        pa, pb = chain(sa), chain(sb)
        common = [s for s in pa if s in pb]
        assert lca == (common[0] if common else -1)
        assert c == sum(fronts[s, 0] for s in common)
        assert longest == max(sum(fronts[s, 0] for s in pa), sum(fronts[s, 0] for s in pb))
    for q in classes["same_supernode"]:
        assert paths[q, 0] == paths[q, 1] == paths[q, 2]
    for q in classes["ancestor"]:
        assert paths[q, 2] in (paths[q, 0], paths[q, 1]) and paths[q, 0] != paths[q, 1]
    for q in classes["root_from_two_subtrees"]:
        assert paths[q, 2] not in (paths[q, 0], paths[q, 1]) and fronts[paths[q, 2], 1] == 0
    for q in classes["folded_landmark_unobserved"]:
        assert fronts[paths[q, 1], 6] == 1


@pytest.mark.parametrize("which,solver,leaf", [("c1", SCHUR, 0), ("c1", SUPERNODAL, 0), ("edge_cases", SCHUR, 0)])
def test_edges_as_queries(which, solver, leaf):
    """The problem's own edges as queries agree with plan_mf_edge_covariances: cross blocks within tol,
    projected ones within 2 tol, in the reference's scales; the diagonal blocks with its marginals."""
    P, _, _, _, _, ref0, vals, _ = _run(which, solver, leaf)
    a = np.concatenate([P.b_pose, P.o_src]).astype(np.int32)
    b = np.concatenate([P.b_lm + P.NP, P.o_dst]).astype(np.int32)
    out = bos.plan_mf_pair_covariances(P, vals, a, b, solver=solver, schur_leaf=leaf)
    edge = bos.plan_mf_edge_covariances(P, vals, solver=solver, schur_leaf=leaf)
    Mb = len(P.b_z)
    sd = np.concatenate([np.sqrt(np.diagonal(edge["pose_cov"], axis1=1, axis2=2)).ravel(),
                         np.sqrt(np.diagonal(edge["landmark_cov"], axis1=1, axis2=2)).ravel()])
    ec = ep = eb = 0.0
    from edge_cov_ref import bearing_jacobians, odometry_jacobians
    Jb = bearing_jacobians(P.pose_xyt[P.b_pose], P.lm_xy[P.b_lm])
    Jo = odometry_jacobians(P.pose_xyt[P.o_src], P.pose_xyt[P.o_dst])
    for q in range(len(a)):
        ia, ib = node_dofs(P, a[q]), node_dofs(P, b[q])
        sc = np.outer(sd[ia], sd[ib])
        C = out["cross"][q, :sc.size].reshape(sc.shape)
        Ce = edge["bearing_cross"][q] if q < Mb else edge["odom_cross"][q - Mb]
        A = out["cov_a"][q, :len(ia) ** 2].reshape(len(ia), len(ia))
        Ae = edge["pose_cov"][a[q]]
        if q < Mb:
            s = (np.abs(Jb[q]) * sd[ia + ib]).sum()
            pe, pscale = abs(out["projected"][q, 0] - edge["bearing_var"][q]), s * s
        else:
            s = (np.abs(Jo[q - Mb]) * sd[ia + ib]).sum(axis=1)
            pe, pscale = np.abs(out["projected"][q].reshape(3, 3) - edge["odom_cov"][q - Mb]), np.outer(s, s)
        nz = sc > 0
        assert np.all(C[~nz] == 0.0) and np.all(Ce[~nz] == 0.0)
        ec = max(ec, float((np.abs(C - Ce)[nz] / sc[nz]).max()) if nz.any() else 0.0)
        pe, pscale = np.atleast_1d(pe), np.atleast_1d(pscale)
        assert np.all(pe[pscale == 0] == 0.0)
        ep = max(ep, float((pe[pscale > 0] / pscale[pscale > 0]).max()) if (pscale > 0).any() else 0.0)
        if a[q] != P.fixed:
            eb = max(eb, float((np.abs(A - Ae) / np.outer(sd[ia], sd[ia])).max()))
    print(f"pair covariances host, edges as queries {which} solver {solver}: tol {ref0.tol:.3g} blocks {eb:.3g} cross {ec:.3g} "
          f"projected {ep:.3g}")
    assert eb <= ref0.tol and ec <= ref0.tol and ep <= 2 * ref0.tol


def test_independent_of_company():
    """A query's bits do not depend on the other pairs of the call."""
    P, a, b, _, out, _, vals, _ = _run("c1", SCHUR, 0)
    for q in (0, 250, 450, len(a) - 1):
        alone = bos.plan_mf_pair_covariances(P, vals, a[q:q + 1], b[q:q + 1], solver=SCHUR)
        assert all(np.array_equal(alone[k][0], out[k][q]) for k in KEYS)


def test_bad_ids_and_empty():
    P, _, _ = _case("mini")
    info = bos.plan_inspect(P, 0, 1, entries=True, solver=SCHUR)
    vals = np.ones(len(info["rows"]))
    for a, b in (([-1], [0]), ([0], [P.NP + P.NL]), ([P.NP], [0])):      # out of range twice; (landmark, pose)
        with pytest.raises(bos.BosError, match=r"\(-1\)"):
            bos.plan_mf_pair_covariances(P, vals, a, b, solver=SCHUR)
        with pytest.raises(bos.BosError, match=r"\(-1\)"):
            bos.plan_pair_paths(P, a, b, solver=SCHUR)
    out = bos.plan_mf_pair_covariances(P, vals, [], [], solver=SCHUR)
    assert all(out[k].shape == (0, 9) for k in KEYS)
    assert bos.plan_pair_paths(P, [], [], solver=SCHUR).shape == (0, 5)
    da, db = dims(P, [0, P.NP], [P.NP, P.NP])
    assert da.tolist() == [3, 2] and db.tolist() == [2, 2]
