"""Joint compatibility on the host (bos_plan_mf_joint_compatibility: the pair hook's path solves and products
over HostMf's factor, then S, its LDL^T and the prefix NIS by csrc/host/joint.hpp) against a dense inverse of
the oracle's H_nf, on the systems of test_pair_cov_host.py. Reference, hypotheses and bounds: tests/joint_ref.py."""
import numpy as np
import pytest

import bos
from joint_ref import JointReference, check_exact_rules, check_recurrence, ldl_prefix, make_hypotheses, s_offdiag
from test_pair_cov_host import PLANS, SCHUR, _case

_cache = {}


def _run(which, solver, leaf=0):
    key = (which, solver, leaf)
    if key not in _cache:
        P, Hl, dense = _case(which)
        info = bos.plan_inspect(P, 0, 1, entries=True, solver=solver, schur_leaf=leaf)
        vals = np.asarray(Hl[info["rows"], info["cols"]]).ravel()
        H = make_hypotheses(P, (P.pose_xyt, P.lm_xy), solver, leaf)

        def run(start, pose, landmark, z, omega, batch=0):
            return bos.plan_mf_joint_compatibility(P, vals, (start, pose, landmark), z, omega, solver=solver, schur_leaf=leaf,
                                                   max_batch=batch)

        _cache[key] = (P, Hl, dense, vals, H, run)
    return _cache[key]


@pytest.mark.parametrize("which,solver,leaf", PLANS)
def test_accuracy(which, solver, leaf):
    """S, e and every prefix NIS within the reference's bounds, and the recurrence reproduced bit for bit."""
    P, Hl, dense, _, H, run = _run(which, solver, leaf)
    out = run(*H.arrays())
    ref = JointReference(P, Hl, *H.arrays(), dense=dense)
    ref.check(out, f"host {which} solver {solver} leaf {leaf}")
    check_recurrence(out)


@pytest.mark.parametrize("which,solver,leaf", [("mini", SCHUR, 0), ("c1", SCHUR, 0), ("c1", SCHUR, 40), ("edge_cases", SCHUR, 0)])
def test_exact_rules(which, solver, leaf):
    """Two calls, prefixes, the repeat, order, company and one hypothesis per batch: identical bits."""
    _, _, _, _, H, run = _run(which, solver, leaf)
    out = check_exact_rules(H, run)
    assert out["joint_nis"][H.index["empty"]] == 0.0


def test_diagonal_and_blocks_from_the_pair_hook():
    """S_ii - 1 / omega_i is the pair hook's projected[0] of (pose_i, NP + landmark_i), bit for bit; an off-diagonal
    entry is s_offdiag of the pair hook's blocks and the Jacobians, within 64 eps s_i s_j (J is not returned: the
    restatement evaluates its own)."""
    from edge_cov_ref import bearing_jacobians
    P, _, _, vals, H, run = _run("c1", SCHUR, 0)
    out = run(*H.arrays())
    for name in ("three_poses", "m32_random", "fixed_pose", "shared_landmark", "pairing_twice"):
        h = H.index[name]
        p, l, _, om = H.one(h)
        S = out["innovation_cov"][h]
        pc = bos.plan_mf_pair_covariances(P, vals, p, P.NP + l, solver=SCHUR)
        assert np.array_equal(np.diag(S), pc["projected"][:, 0] + 1.0 / om), name
        J = bearing_jacobians(P.pose_xyt[p], P.lm_xy[l])
        nodes = np.stack([p, P.NP + l], axis=1)
        for i in range(1, min(len(p), 6)):
            for j in range(i):
                C = np.zeros((5, 5))
                sd = []
                for bi, u in enumerate(nodes[i]):
                    for bj, v in enumerate(nodes[j]):
                        a, b = (u, v) if u <= v else (v, u)
                        q = bos.plan_mf_pair_covariances(P, vals, [a], [b], solver=SCHUR)
                        da, db = (3 if a < P.NP else 2), (3 if b < P.NP else 2)
                        blk = (q["cov_a"] if a == b else q["cross"])[0, :da * db].reshape(da, db)
                        blk = blk if u <= v else blk.T
                        C[3 * bi:3 * bi + blk.shape[0], 3 * bj:3 * bj + blk.shape[1]] = blk
                for u in (nodes[i], nodes[j]):
                    q = bos.plan_mf_pair_covariances(P, vals, [u[0]], [u[1]], solver=SCHUR)
                    sd.append(np.sqrt(np.concatenate([np.diag(q["cov_a"][0].reshape(3, 3)), np.diag(q["cov_b"][0, :4].reshape(2, 2))])))
                si, sj = (np.abs(J[i]) * sd[0]).sum(), (np.abs(J[j]) * sd[1]).sum()
                assert abs(S[i, j] - s_offdiag(C, J[i], J[j])) <= 64 * 2.22e-16 * si * sj, (name, i, j)


def test_pivots_and_restatement():
    """ldl_prefix on matrices that are not positive definite: NaN from the first bad pivot on."""
    S = np.array([[2.0, 1.0, 0.0], [1.0, 0.5, 0.0], [0.0, 0.0, 1.0]])      # D_1 = 0
    out = ldl_prefix(S, np.array([1.0, 1.0, 1.0]))
    assert out[0] == 0.5 and np.isnan(out[1]) and np.isnan(out[2])
    assert np.all(np.isnan(ldl_prefix(np.array([[-1.0]]), np.array([1.0]))))
    assert s_offdiag(np.eye(5), np.arange(5.0), np.ones(5)) == 10.0


def test_argument_errors_leave_the_outputs():
    P, _, _, vals, _, _ = _run("mini", SCHUR, 0)
    cs, opt = P.c_struct(), bos.options(SCHUR)
    import ctypes
    L = bos.lib()
    dp, ip = ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_int32)
    v = np.ascontiguousarray(vals)
    m_big = bos.JOINT_MAX_M + 1
    cases = {"start_not_zero": ([1, 2], [0, 0], [0, 0], [0.1, 0.1], None),
             "decreasing": ([0, 2, 1], [0, 0], [0, 0], [0.1, 0.1], None),
             "too_large": ([0, m_big], [0] * m_big, [0] * m_big, [0.1] * m_big, None),
             "pose_low": ([0, 1], [-1], [0], [0.1], None),
             "pose_high": ([0, 1], [P.NP], [0], [0.1], None),
             "landmark_low": ([0, 1], [0], [-1], [0.1], None),
             "landmark_high": ([0, 1], [0], [P.NL], [0.1], None),
             "z_nan": ([0, 1], [0], [0], [np.nan], None),
             "z_inf": ([0, 1], [0], [0], [np.inf], None),
             "omega_zero": ([0, 1], [0], [0], [0.1], [0.0]),
             "omega_negative": ([0, 1], [0], [0], [0.1], [-1.0]),
             "omega_nan": ([0, 1], [0], [0], [0.1], [np.nan]),
             "omega_inf": ([0, 1], [0], [0], [0.1], [np.inf])}
    for name, (start, pose, lm, z, om) in cases.items():
        start, pose, lm = (np.array(x, dtype=np.int32) for x in (start, pose, lm))
        z = np.array(z)
        om = None if om is None else np.array(om)
        outs = [np.full(64, 7.0) for _ in range(3)] + [np.full(2048, 7.0)]
        rc = L.bos_plan_mf_joint_compatibility(ctypes.byref(cs), ctypes.byref(opt), v.ctypes.data_as(dp), len(start) - 1,
                                               start.ctypes.data_as(ip), pose.ctypes.data_as(ip), lm.ctypes.data_as(ip),
                                               z.ctypes.data_as(dp), None if om is None else om.ctypes.data_as(dp), 0,
                                               *[o.ctypes.data_as(dp) for o in outs])
        assert rc == -1, name
        assert all(np.all(o == 7.0) for o in outs), name
    out = bos.plan_mf_joint_compatibility(P, vals, [], solver=SCHUR)
    assert len(out["joint_nis"]) == 0 and out["innovation_cov"] == []
    # the list form and the flat form are the same call; omega None is 1 everywhere
    x = bos.plan_mf_joint_compatibility(P, vals, [([1, 2], [0, 1], [0.1, 0.2])], solver=SCHUR)
    y = bos.plan_mf_joint_compatibility(P, vals, ([0, 2], [1, 2], [0, 1]), [0.1, 0.2], [1.0, 1.0], solver=SCHUR)
    assert np.array_equal(x["prefix_nis"], y["prefix_nis"]) and np.array_equal(x["innovation_cov"][0], y["innovation_cov"][0])
