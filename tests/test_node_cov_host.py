"""Node covariances on the host (bos_plan_mf_node_covariances: per query node the root-path solve, the
scatter into X, the backward sweep over every front of HostMf's factor, the gather and the projection of
csrc/host/node_cov.hpp) against a dense inverse of the oracle's H_nf. Query nodes, the conversion to the
pair layout and the exact rules: tests/node_cov_ref.py; reference, error measures and bounds:
tests/pair_cov_ref.py."""
import numpy as np
import pytest

import bos
import oracle as O
from conftest import C1, MINI
from helpers import oracle_lower_nf, to_oracle
from marginals_ref import DenseInverses
from node_cov_ref import NODE_KEYS, check_column_rules, query_nodes, to_pairs
from pair_cov_ref import PairReference, check_reference, check_refined
from test_edge_cov_host import edge_case_world

SCHUR, SUPERNODAL = bos.BOS_SOLVER_SCHUR, bos.BOS_SOLVER_SUPERNODAL

_cache = {}


def _case(which):
    """Problem, the oracle's lower H_nf (damping 0.01) and its dense inverses: once per world."""
    if which not in _cache:
        if which == "synthetic":
            P = bos.synthetic(60, 120, 6)
        else:
            P = bos.load_g2o(MINI if which == "mini" else C1)
        if which == "edge_cases":
            P = edge_case_world(P)
        Q = to_oracle(P)
        Hl = oracle_lower_nf(Q, O.linearize(Q, damping=0.01)).tocsr()
        _cache[which] = (P, Hl, DenseInverses(P, Hl))
    return _cache[which]


def _run(which, solver, leaf=0):
    key = (which, solver, leaf)
    if key not in _cache:
        P, Hl, dense = _case(which)
        nodes, kinds = query_nodes(P, solver, leaf)
        info = bos.plan_inspect(P, 0, 1, entries=True, solver=solver, schur_leaf=leaf)
        vals = np.asarray(Hl[info["rows"], info["cols"]]).ravel()
        out = bos.plan_mf_node_covariances(P, vals, nodes, solver=solver, schur_leaf=leaf)
        _cache[key] = (P, nodes, kinds, out, vals, info)
    return _cache[key]


PLANS = [("mini", SCHUR, 0), ("mini", SUPERNODAL, 0), ("c1", SCHUR, 0), ("c1", SUPERNODAL, 0), ("c1", SCHUR, 40),
         ("edge_cases", SCHUR, 0), ("edge_cases", SUPERNODAL, 0), ("synthetic", SCHUR, 0)]


@pytest.mark.parametrize("which,solver,leaf", PLANS)
def test_accuracy(which, solver, leaf):
    """Every block of the queried columns: reference bounds, the refined criterion and the exact rules."""
    P, nodes, kinds, out, _, info = _run(which, solver, leaf)
    _, Hl, dense = _case(which)
    a, b, pairs = to_pairs(P, nodes, out)
    ref = PairReference(P, Hl, a, b, dense=dense)
    label = f"node column host {which} solver {solver} leaf {leaf} max front {info['mf_max_front']} queries {','.join(kinds)}"
    check_reference(ref, pairs, label)
    check_refined(ref, pairs, label)
    check_column_rules(P, nodes, out)


@pytest.mark.parametrize("which,solver,leaf", [("c1", SCHUR, 0), ("c1", SUPERNODAL, 0), ("synthetic", SCHUR, 0)])
def test_query_kinds(which, solver, leaf):
    """The worlds show every kind of query node their plan can have."""
    P, nodes, kinds, _, _, _ = _run(which, solver, leaf)
    fronts = bos.plan_mf_fronts(P, solver=solver, schur_leaf=leaf)
    for k in ("fixed_pose", "leaf_pose", "root_pose", "last_pose", "repeated"):
        assert k in kinds, k
    assert ("folded_landmark" in kinds) == bool(fronts[:, 6].any())
    assert nodes[0] == P.fixed and nodes[-1] == nodes[1]


def test_marginals_are_the_selected_inverse():
    """pose_cov / landmark_cov are plan_mf_marginals' bits."""
    P, _, _, out, vals, _ = _run("c1", SCHUR, 0)
    pose, lm = bos.plan_mf_marginals(P, vals, solver=SCHUR)
    assert np.array_equal(out["pose_cov"], pose) and np.array_equal(out["landmark_cov"], lm)


def test_agrees_with_pair_covariances():
    """The same column through plan_mf_pair_covariances: cross within tol, projected within 2 tol, in the
    reference's scales."""
    P, nodes, _, out, vals, _ = _run("c1", SCHUR, 0)
    _, Hl, dense = _case("c1")
    a, b, pairs = to_pairs(P, nodes, out)
    ref = PairReference(P, Hl, a, b, dense=dense)
    pair = bos.plan_mf_pair_covariances(P, vals, a, b, solver=SCHUR)
    e = {}
    for k in ("cross", "projected"):
        sc = ref.scale[k].astype(np.float64)
        d = np.abs(pairs[k] - pair[k])
        assert np.all(d[sc == 0] == 0.0)
        e[k] = float((d[sc > 0] / sc[sc > 0]).max())
    print(f"node column host vs pair route c1: tol {ref.tol:.3g} cross {e['cross']:.3g} projected {e['projected']:.3g}")
    assert e["cross"] <= ref.tol and e["projected"] <= 2 * ref.tol


def test_independent_of_company():
    """A query's bits do not depend on the other nodes of the call."""
    P, nodes, _, out, vals, _ = _run("c1", SCHUR, 0)
    for i in (1, len(nodes) - 3):
        alone = bos.plan_mf_node_covariances(P, vals, nodes[i:i + 1], solver=SCHUR)
        assert all(np.array_equal(alone[k][0], out[k][i]) for k in NODE_KEYS)


def test_bad_ids_and_empty():
    P, _, _ = _case("mini")
    info = bos.plan_inspect(P, 0, 1, entries=True, solver=SCHUR)
    vals = np.ones(len(info["rows"]))
    for nodes in ([-1], [P.NP + P.NL], [0, P.NP + P.NL]):
        with pytest.raises(bos.BosError, match=r"\(-1\)"):
            bos.plan_mf_node_covariances(P, vals, nodes, solver=SCHUR)
    out = bos.plan_mf_node_covariances(P, vals, [], solver=SCHUR)
    assert out["cross_pose"].shape == (0, P.NP, 9) and out["projected_landmark"].shape == (0, P.NL, 4)
