"""Shared by the node-covariance tests (host and GPU): the query nodes of a world, the conversion of a
bos_node_covariances result to the pair layout, so that the reference, the error measures and the bounds of
tests/pair_cov_ref.py (PairReference, check_reference, check_refined) are used unchanged, and the exact
rules of the column call.

Outputs (bos.h bos_node_covariances), query i with a = nodes[i] of d_a dofs: cross_pose [n, NP, 9] and
cross_landmark [n, NL, 6] hold Sigma(a, u), d_a x d_u row-major in the first entries of the slot;
projected_pose [n, NP, 9] and projected_landmark [n, NL, 4] the projection of the pair. Pair layout: query a
against target u is the pair (a, u), or (u, a) with the cross block transposed where a is a landmark and u a
pose (a mixed pair is written (pose, landmark)); cov_a / cov_b are the call's own marginals."""
import numpy as np

import bos
from pair_cov_ref import KEYS

NODE_KEYS = ("cross_pose", "cross_landmark", "projected_pose", "projected_landmark")


def query_nodes(P, solver, schur_leaf=0):
    """(nodes, kinds): the fixed pose, a pose in a leaf front, a pose in a root supernode, the last pose, a
    folded landmark and a non-folded one where the plan has them, and the leaf pose once more (a repeated
    id). kinds names what was found."""
    ids = np.arange(P.NP + P.NL, dtype=np.int32)
    sn = bos.plan_pair_paths(P, ids, ids, solver=solver, schur_leaf=schur_leaf)[:, 0]
    fronts = bos.plan_mf_fronts(P, solver=solver, schur_leaf=schur_leaf)
    free = sn >= 0
    leaf = np.zeros(len(ids), dtype=bool)
    root = np.zeros(len(ids), dtype=bool)
    folded = np.zeros(len(ids), dtype=bool)
    leaf[free] = (fronts[sn[free], 4] == fronts[sn[free], 5]) & (fronts[sn[free], 6] == 0)   # folded children at most
    root[free] = (fronts[sn[free], 3] < 0) | (fronts[sn[free], 1] == 0)
    folded[free] = fronts[sn[free], 6] == 1
    pose = ids < P.NP
    nodes, kinds = [int(P.fixed)], ["fixed_pose"]

    def first(name, mask):
        idx = np.nonzero(mask)[0]
        if len(idx):
            nodes.append(int(idx[0]))
            kinds.append(name)

    first("leaf_pose", pose & leaf)
    first("root_pose", pose & root)
    last = P.NP - 1 if P.fixed != P.NP - 1 else P.NP - 2
    nodes.append(last)
    kinds.append("last_pose")
    first("folded_landmark", ~pose & folded)
    first("unfolded_landmark", ~pose & free & ~folded)
    nodes.append(nodes[1])
    kinds.append("repeated")
    return np.array(nodes, dtype=np.int32), kinds


def to_pairs(P, nodes, out):
    """(node_a, node_b, pair-layout dict over KEYS) of a node-covariance result with all outputs."""
    NP, NL = P.NP, P.NL
    n = len(nodes) * (NP + NL)
    node_a, node_b = np.zeros(n, dtype=np.int32), np.zeros(n, dtype=np.int32)
    pairs = {k: np.zeros((n, 9)) for k in KEYS}

    def block(u):
        return out["pose_cov"][u].ravel() if u < NP else out["landmark_cov"][u - NP].ravel()

    q = 0
    for i, a in enumerate(int(x) for x in nodes):
        da = 3 if a < NP else 2
        for u in range(NP + NL):
            du = 3 if u < NP else 2
            C = (out["cross_pose"][i, u] if u < NP else out["cross_landmark"][i, u - NP])[:da * du].reshape(da, du)
            proj = out["projected_pose"][i, u] if u < NP else out["projected_landmark"][i, u - NP]
            swap = a >= NP and u < NP
            node_a[q], node_b[q] = (u, a) if swap else (a, u)
            Cq = C.T if swap else C
            pairs["cross"][q, :Cq.size] = Cq.ravel()
            pairs["projected"][q, :proj.size] = proj
            ba, bb = block(node_a[q]), block(node_b[q])
            pairs["cov_a"][q, :ba.size] = ba
            pairs["cov_b"][q, :bb.size] = bb
            q += 1
    return node_a, node_b, pairs


def check_column_rules(P, nodes, out):
    """The exact rules of bos_node_covariances on one result (all four node outputs): zeros outside the
    blocks, the fixed pose as query and as target, the projected entry of u == a, repeated ids."""
    NP, fx = P.NP, P.fixed
    cp, cl, pp, pl = (out[k] for k in NODE_KEYS)
    for i, a in enumerate(int(x) for x in nodes):
        da = 3 if a < NP else 2
        assert np.all(cp[i, :, da * 3:] == 0.0) and np.all(cl[i, :, da * 2:] == 0.0)
        if a < NP:
            assert np.all(pl[i, :, 1:] == 0.0)                       # a bearing's variance in entry 0
            M = pp[i].reshape(NP, 3, 3)
            assert np.array_equal(M, M.transpose(0, 2, 1))           # lower triangle mirrored
        else:
            assert np.all(pp[i, :, 1:] == 0.0)
            M = pl[i].reshape(-1, 2, 2)
            assert np.array_equal(M, M.transpose(0, 2, 1))
            assert np.all(pl[i, a - NP] == 0.0)                      # l_a - l_a
        if a == fx:
            assert np.all(cp[i] == 0.0) and np.all(cl[i] == 0.0)
            assert np.all(pp[i, fx] == 0.0)                          # nothing free is involved
        else:
            own = (cp[i, a, :9] if a < NP else cl[i, a - NP, :4]).reshape(da, da)
            assert np.all(np.diag(own) > 0.0)
        assert np.all(cp[i, fx] == 0.0)
    seen = {}
    for i, a in enumerate(int(x) for x in nodes):
        f = seen.setdefault(a, i)
        if f != i:
            assert all(np.array_equal(out[k][i], out[k][f]) for k in NODE_KEYS), (i, f)
