"""Node matching on the host (bos_plan_mf_match_landmarks / bos_plan_mf_match_poses: per distinct query node
the node column's projected slice over HostMf's factor, then the scores by csrc/host/match.hpp and a plain
sort) against tests/match_ref.py at a dense inverse of the oracle's H_nf: the rows within the reference's
bound, the selection and the counts exactly against a stable sort of the twin's own rows with every listed
score reproduced in NumPy from its listed details, the exact rules, R against np.linalg.inv and the argument
rules."""
import ctypes

import numpy as np
import pytest

import bos
import oracle as O
from conftest import C1, MINI
from helpers import EPS, oracle_lower_nf, to_oracle
from marginals_ref import DenseInverses
from match_ref import (LM_KEYS, OMEGAS, POSE_KEYS, LandmarkReference, PoseReference, check_landmark_selection, check_pose_selection,
                       make_measurements, query_landmarks, query_poses)
from test_edge_cov_host import edge_case_world

SCHUR, SUPERNODAL = bos.BOS_SOLVER_SCHUR, bos.BOS_SOLVER_SUPERNODAL
ERR_INVALID = -1   # include/bos.h BOS_ERR_INVALID

_cache = {}


def _case(which):
    """Problem, the oracle's lower H_nf (damping 0.01), the queries and their references: once per world. The
    query nodes include the fixed pose, the first and the last pose, the first, a middle and the last landmark."""
    if which not in _cache:
        if which == "synthetic":
            P = bos.synthetic(60, 120, 6)
        else:
            P = bos.load_g2o(MINI if which == "mini" else C1)
            if which == "edge_cases":
                P = edge_case_world(P)
        Q = to_oracle(P)
        Hl = oracle_lower_nf(Q, O.linearize(Q, damping=0.01)).tocsr()
        dense = DenseInverses(P, Hl)
        lms = np.array(query_landmarks(P), dtype=np.int32)
        pose, z, omega = make_measurements(P, P.pose_xyt, query_poses(P))
        _cache[which] = dict(P=P, Hl=Hl, lms=lms, pose=pose, z=z, omega=omega, lm_ref=LandmarkReference(P, Hl, lms, dense=dense),
                             pose_ref=PoseReference(P, Hl, pose, z, omega, dense=dense))
    return _cache[which]


def _vals(which, solver=SCHUR, leaf=0):
    c = _case(which)
    info = bos.plan_inspect(c["P"], 0, 1, entries=True, solver=solver, schur_leaf=leaf)
    return np.asarray(c["Hl"][info["rows"], info["cols"]]).ravel()


PLANS = [("mini", SCHUR, 0), ("mini", SUPERNODAL, 0), ("c1", SCHUR, 0), ("c1", SUPERNODAL, 0), ("c1", SCHUR, 40),
         ("edge_cases", SCHUR, 0), ("synthetic", SCHUR, 0)]


@pytest.mark.parametrize("which", ["mini", "c1", "edge_cases", "synthetic"])
def test_reference_is_well_conditioned(which):
    """tol_M |M^-1|_2 <= 0.1 for both gates and the wrap cap, on the reference alone; the measurements do hold
    an angle error near the wrap."""
    c = _case(which)
    c["lm_ref"].check_condition(f"landmarks {which}")
    c["pose_ref"].check_condition(f"poses {which}")
    assert (np.abs(np.abs(c["pose_ref"].e[:, :, 2]) - np.pi) < 0.05).any()


@pytest.mark.parametrize("which,solver,leaf", PLANS)
def test_landmark_rows_against_reference(which, solver, leaf):
    c = _case(which)
    out = bos.plan_mf_match_landmarks(c["P"], _vals(which, solver, leaf), c["lms"], solver=solver, schur_leaf=leaf)
    c["lm_ref"].check_scores(out["d2_all"], f"host landmarks {which} solver {solver} leaf {leaf}")
    for q, a in enumerate(c["lms"]):
        assert np.isnan(out["d2_all"][q, a]) and a not in out["cand_landmark"][q]
    assert np.all(out["n_inside"] == c["P"].NL - 1)


@pytest.mark.parametrize("which,solver,leaf", PLANS)
def test_pose_rows_against_reference(which, solver, leaf):
    c = _case(which)
    out = bos.plan_mf_match_poses(c["P"], _vals(which, solver, leaf), c["pose"], c["z"], c["omega"], solver=solver, schur_leaf=leaf)
    c["pose_ref"].check_scores(out["nis_all"], f"host poses {which} solver {solver} leaf {leaf}")


@pytest.mark.parametrize("k", [1, 4, 8])
@pytest.mark.parametrize("which", ["mini", "c1"])
def test_selection_is_exact(which, k):
    """cand_* and n_inside against the twin's own rows: gate +inf, a gate that passes a handful, a gate below
    every score; cand_cov is the node hook's block (plus R for poses) in its bits; the listed scores by the
    recipe from the listed details."""
    c = _case(which)
    P, vals = c["P"], _vals(which)
    node = bos.plan_mf_node_covariances(P, vals, list(P.NP + c["lms"]) + sorted(set(c["pose"].tolist())))
    n_lm = len(c["lms"])
    full = bos.plan_mf_match_landmarks(P, vals, c["lms"], k=k)
    rows = full["d2_all"]
    handful = float(np.sort(rows, axis=1)[:, min(2, P.NL - 2)].max())
    for gate in (np.inf, handful, float(np.nanmin(rows)) / 2):
        out = bos.plan_mf_match_landmarks(P, vals, c["lms"], gate=gate, k=k)
        assert np.array_equal(out["d2_all"], rows, equal_nan=True)
        check_landmark_selection(out, gate, k)
        for q in range(n_lm):
            listed = out["cand_landmark"][q] >= 0
            l = out["cand_landmark"][q][listed]
            assert np.array_equal(out["cand_cov"][q][listed], node["projected_landmark"][q, l])
            assert np.array_equal(out["cand_diff"][q][listed], P.lm_xy[c["lms"][q]] - P.lm_xy[l])
    assert np.all(out["n_inside"] == 0) and np.all(out["cand_landmark"] == -1)         # the last gate lists nothing
    if which == "mini":
        assert P.NL < 8 and (k < 8 or np.all(full["cand_landmark"][:, P.NL - 1:] == -1))   # padding past NL - 1
    distinct = sorted(set(c["pose"].tolist()))
    full = bos.plan_mf_match_poses(P, vals, c["pose"], c["z"], c["omega"], k=k)
    rows = full["nis_all"]
    handful = float(np.sort(rows, axis=1)[:, min(2, P.NP - 1)].max())
    for gate in (np.inf, handful, float(rows.min()) / 2):
        out = bos.plan_mf_match_poses(P, vals, c["pose"], c["z"], c["omega"], gate=gate, k=k)
        assert np.array_equal(out["nis_all"], rows)
        check_pose_selection(out, gate, k)
        for q in range(len(c["pose"])):
            listed = out["cand_pose"][q] >= 0
            Pm = node["projected_pose"][n_lm + distinct.index(int(c["pose"][q])), out["cand_pose"][q][listed]]
            S = Pm + bos.match_information_inverse(c["omega"][q]).ravel()
            low = [0, 3, 4, 6, 7, 8]
            assert np.array_equal(out["cand_cov"][q][listed][:, low], S[:, low])
    assert np.all(out["n_inside"] == 0) and np.all(out["cand_pose"] == -1)


def test_exact_rules():
    """A query's bits depend neither on its company nor on the order; a repeated query returns identical
    bits; omega None is the identity; two calls give identical bits."""
    c = _case("c1")
    P, vals = c["P"], _vals("c1")
    lms = np.concatenate([c["lms"], c["lms"][:1]])
    a = bos.plan_mf_match_landmarks(P, vals, lms, gate=50.0)
    b = bos.plan_mf_match_landmarks(P, vals, lms[::-1], gate=50.0)
    one = bos.plan_mf_match_landmarks(P, vals, lms[1:2], gate=50.0)
    for key in LM_KEYS:
        assert np.array_equal(a[key], b[key][::-1], equal_nan=True) and np.array_equal(a[key][0], a[key][-1], equal_nan=True)
        assert np.array_equal(one[key][0], a[key][1], equal_nan=True)
    pose, z, omega = c["pose"], c["z"], c["omega"]
    a = bos.plan_mf_match_poses(P, vals, pose, z, omega, gate=50.0)
    b = bos.plan_mf_match_poses(P, vals, pose[::-1], z[::-1], omega[::-1], gate=50.0)
    again = bos.plan_mf_match_poses(P, vals, pose, z, omega, gate=50.0)
    one = bos.plan_mf_match_poses(P, vals, pose[5:6], z[5:6], omega[5:6], gate=50.0)
    for key in POSE_KEYS:
        assert np.array_equal(a[key], b[key][::-1]) and np.array_equal(a[key], again[key]) and np.array_equal(one[key][0], a[key][5])
        for q in range(0, len(pose), 4):                                              # entry 3 repeats entry 0
            assert np.array_equal(a[key][q], a[key][q + 3])
    x = bos.plan_mf_match_poses(P, vals, pose, z, None)
    y = bos.plan_mf_match_poses(P, vals, pose, z, np.tile(np.eye(3).ravel(), (len(pose), 1)))
    assert all(np.array_equal(x[key], y[key]) for key in POSE_KEYS)


def test_information_inverse():
    """R against np.linalg.inv within 64 eps kappa |R|, bit-symmetric, the identity exactly; what is refused."""
    for name, om in OMEGAS.items():
        R = bos.match_information_inverse(om)
        ref = np.linalg.inv(om)
        assert np.array_equal(R, R.T)
        assert np.abs(R - ref).max() <= 64 * EPS * np.linalg.cond(om) * np.abs(ref).max(), name
    assert np.array_equal(bos.match_information_inverse(np.eye(3)), np.eye(3))
    asym = OMEGAS["full"].copy()
    asym[0, 1] = np.nextafter(asym[0, 1], 1e9)
    indefinite = np.array([[1.0, 2.0, 0.0], [2.0, 1.0, 0.0], [0.0, 0.0, 1.0]])
    nan = OMEGAS["diag"].copy()
    nan[2, 2] = np.nan
    for om in (asym, indefinite, nan, np.zeros((3, 3)), -np.eye(3)):
        with pytest.raises(bos.BosError, match=r"\(-1\)"):
            bos.match_information_inverse(om)


def _raw(P, vals, which, args, gate, k, fill=7):
    """The C call with sentinel-filled outputs: (rc, outputs)."""
    cs = P.c_struct()
    opt = bos.options(SCHUR)
    dp, ip = ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_int32)
    ptr = lambda x: None if x is None else x.ctypes.data_as(ip if x.dtype == np.int32 else dp)
    n, kk = len(args[0]), 8
    dd, dc, N = (2, 4, P.NL) if which == "landmarks" else (3, 9, P.NP)
    outs = [np.full((n, kk), fill, dtype=np.int32), np.full((n, kk), float(fill)), np.full((n, kk, dd), float(fill)),
            np.full((n, kk, dc), float(fill)), np.full(n, fill, dtype=np.int32), np.full((n, N), float(fill))]
    ins = [np.ascontiguousarray(args[0], dtype=np.int32)] + [None if x is None else np.ascontiguousarray(x, dtype=np.float64) for x in args[1:]]
    f = bos.lib().bos_plan_mf_match_landmarks if which == "landmarks" else bos.lib().bos_plan_mf_match_poses
    rc = f(ctypes.byref(cs), ctypes.byref(opt), ptr(vals), n, *[ptr(x) for x in ins], gate, k, *[ptr(o) for o in outs])
    return rc, outs


def test_invalid_arguments_touch_nothing():
    c = _case("mini")
    P, vals = c["P"], _vals("mini")
    lms, pose, z, omega = c["lms"], c["pose"], c["z"], c["omega"]
    bad_lm = lms.copy()
    bad_lm[1] = P.NL
    for case in [((bad_lm,), 1.0, 4), ((-lms - 1,), 1.0, 4), ((lms,), np.nan, 4), ((lms,), 0.0, 4), ((lms,), -1.0, 4), ((lms,), 1.0, 0),
                 ((lms,), 1.0, 9)]:
        rc, outs = _raw(P, vals, "landmarks", *case)
        assert rc == ERR_INVALID and all(np.all(o == 7) for o in outs), case
    bad_pose, bad_z, nan_om, asym_om, neg_om = pose.copy(), z.copy(), omega.copy(), omega.copy(), omega.copy()
    bad_pose[1] = P.NP
    bad_z[2, 1] = np.inf
    nan_om[0, 4] = np.nan
    asym_om[1, 1] = np.nextafter(asym_om[1, 1], 1e9)                                  # entry (0, 1) without (1, 0)
    neg_om[3] = -np.eye(3).ravel()
    for case in [((bad_pose, z, omega), 1.0, 4), ((-pose - 1, z, omega), 1.0, 4), ((pose, bad_z, omega), 1.0, 4),
                 ((pose, z, nan_om), 1.0, 4), ((pose, z, asym_om), 1.0, 4), ((pose, z, neg_om), 1.0, 4), ((pose, z, omega), np.nan, 4),
                 ((pose, z, omega), 0.0, 4), ((pose, z, omega), 1.0, 0), ((pose, z, omega), 1.0, 9)]:
        rc, outs = _raw(P, vals, "poses", *case)
        assert rc == ERR_INVALID and all(np.all(o == 7) for o in outs), case
    assert _raw(P, vals, "landmarks", (lms[:0],), 1.0, 4)[0] == bos.BOS_OK              # n == 0
    assert _raw(P, vals, "poses", (pose[:0], z[:0], None), 1.0, 4)[0] == bos.BOS_OK
    rc, outs = _raw(P, vals, "poses", (pose, z, omega), np.inf, 8)
    assert rc == bos.BOS_OK and not any(np.any(o == 7) for o in outs[:5]) and outs[4][0] == P.NP
