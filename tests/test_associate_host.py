"""Bearing association on the host (bos_plan_mf_associate_bearings: per distinct pose the node column's
projected_landmark over HostMf's factor, then e, S and nis by csrc/host/associate.hpp and a plain sort)
against tests/associate_ref.py at a dense inverse of the oracle's H_nf: the NIS rows within the reference's
bound, the selection and the counts exactly against a stable sort of the twin's own rows, and the argument
rules."""
import ctypes

import numpy as np
import pytest

import bos
import oracle as O
from associate_ref import AssocReference, check_selection, expected_selection, make_bearings
from conftest import C1, MINI
from helpers import oracle_lower_nf, to_oracle
from marginals_ref import DenseInverses

SCHUR, SUPERNODAL = bos.BOS_SOLVER_SCHUR, bos.BOS_SOLVER_SUPERNODAL
ERR_INVALID = -1   # include/bos.h BOS_ERR_INVALID

_cache = {}


def _case(which):
    """Problem, the oracle's lower H_nf (damping 0.01), its dense inverses, the test bearings and their
    reference: once per world. The query poses include the fixed pose and the last one."""
    if which not in _cache:
        P = bos.load_g2o(MINI if which == "mini" else C1)
        Q = to_oracle(P)
        Hl = oracle_lower_nf(Q, O.linearize(Q, damping=0.01)).tocsr()
        poses = sorted({P.fixed, 0, P.NP // 2, P.NP - 1})
        pose, z, omega = make_bearings(P, P.pose_xyt, P.lm_xy, poses)
        ref = AssocReference(P, Hl, pose, z, omega, dense=DenseInverses(P, Hl))
        _cache[which] = (P, Hl, pose, z, omega, ref)
    return _cache[which]


def _vals(which, solver, leaf):
    P, Hl = _case(which)[:2]
    info = bos.plan_inspect(P, 0, 1, entries=True, solver=solver, schur_leaf=leaf)
    return np.asarray(Hl[info["rows"], info["cols"]]).ravel()


PLANS = [("mini", SCHUR, 0), ("mini", SUPERNODAL, 0), ("c1", SCHUR, 0), ("c1", SUPERNODAL, 0), ("c1", SCHUR, 40)]


@pytest.mark.parametrize("which,solver,leaf", PLANS)
def test_nis_against_reference(which, solver, leaf):
    P, _, pose, z, omega, ref = _case(which)
    out = bos.plan_mf_associate_bearings(P, _vals(which, solver, leaf), pose, z, omega, solver=solver, schur_leaf=leaf)
    node = bos.plan_mf_node_covariances(P, _vals(which, solver, leaf), ref.distinct, solver=solver, schur_leaf=leaf)
    ref.check_var(node["projected_landmark"][:, :, 0], f"host {which} solver {solver} leaf {leaf}")
    ref.check_nis(out["nis_all"], f"host {which} solver {solver} leaf {leaf}")


@pytest.mark.parametrize("which", ["mini", "c1"])
def test_reference_stays_inside_the_wrap_cap(which):
    """The test bearings leave at most 1 % of the reference's entries within 1e-9 of the wrap, and they do
    hold an innovation near it."""
    ref = _case(which)[5]
    print(f"  association reference {which}: excluded {ref.excluded:.3g}")
    assert ref.excluded <= 0.01
    assert (np.abs(np.abs(ref.e) - np.pi) < 0.05).any()


@pytest.mark.parametrize("k", [1, 4, 8])
@pytest.mark.parametrize("which", ["mini", "c1"])
def test_selection_is_exact(which, k):
    """cand_* and n_inside against the twin's own nis_all: gate +inf, a gate that passes a handful, a gate
    below every NIS; cand_var is the node hook's variance + 1 / omega in its bits."""
    P, _, pose, z, omega, ref = _case(which)
    vals = _vals(which, SCHUR, 0)
    full = bos.plan_mf_associate_bearings(P, vals, pose, z, omega, k=k)
    finite = full["nis_all"][np.isfinite(full["nis_all"])]
    some = float(np.sort(full["nis_all"], axis=1)[:, min(2, P.NL - 1)].max())
    node = bos.plan_mf_node_covariances(P, vals, ref.distinct)["projected_landmark"][:, :, 0]
    for gate in (np.inf, some, float(finite.min()) / 2):
        out = bos.plan_mf_associate_bearings(P, vals, pose, z, omega, gate=gate, k=k)
        assert np.array_equal(out["nis_all"], full["nis_all"])
        check_selection(out, gate, k)
        for q in range(len(pose)):
            listed = out["cand_landmark"][q] >= 0
            var = node[ref.distinct.index(int(pose[q])), out["cand_landmark"][q][listed]]
            assert np.array_equal(out["cand_var"][q][listed], var + 1 / omega[q])
    assert np.all(out["n_inside"] == 0) and np.all(out["cand_landmark"] == -1)       # the last gate lists nothing
    if which == "mini":
        assert P.NL < 8 and (k < 8 or np.all(full["cand_landmark"][:, P.NL:] == -1))   # padding past NL


def test_omega_null_is_one_and_repeats_are_identical():
    P, _, pose, z, omega, _ = _case("c1")
    vals = _vals("c1", SCHUR, 0)
    a = bos.plan_mf_associate_bearings(P, vals, pose, z, None)
    b = bos.plan_mf_associate_bearings(P, vals, pose, z, np.ones(len(pose)))
    assert all(np.array_equal(a[k], b[k]) for k in a)
    out = bos.plan_mf_associate_bearings(P, vals, pose, z, omega)
    for q in range(0, len(pose), 4):                                               # entry 3 repeats entry 0
        assert all(np.array_equal(out[k][q], out[k][q + 3]) for k in out)


def _raw(P, vals, pose, z, omega, gate, k, fill=7):
    """The C call with sentinel-filled outputs: (rc, outputs)."""
    cs = P.c_struct()
    opt = bos.options(SCHUR)
    n = len(pose)
    a, zz = np.asarray(pose, dtype=np.int32), np.asarray(z, dtype=np.float64)
    om = None if omega is None else np.asarray(omega, dtype=np.float64)
    kk = 8
    outs = [np.full((n, kk), fill, dtype=np.int32), np.full((n, kk), float(fill)), np.full((n, kk), float(fill)),
            np.full((n, kk), float(fill)), np.full(n, fill, dtype=np.int32), np.full((n, P.NL), float(fill))]
    dp, ip = ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_int32)
    ptr = lambda x: None if x is None else x.ctypes.data_as(ip if x.dtype == np.int32 else dp)
    rc = bos.lib().bos_plan_mf_associate_bearings(ctypes.byref(cs), ctypes.byref(opt), ptr(vals), n, ptr(a), ptr(zz), ptr(om), gate, k,
                                                  *[ptr(o) for o in outs])
    return rc, outs


def test_invalid_arguments_touch_nothing():
    P, _, pose, z, omega, _ = _case("mini")
    vals = _vals("mini", SCHUR, 0)
    bad_pose, bad_z, bad_om, neg_om = pose.copy(), z.copy(), omega.copy(), omega.copy()
    bad_pose[1] = P.NP
    bad_z[2] = np.inf
    bad_om[0] = np.nan
    neg_om[3] = 0.0
    cases = [(bad_pose, z, omega, 1.0, 4), (-pose - 1, z, omega, 1.0, 4), (pose, bad_z, omega, 1.0, 4), (pose, z, bad_om, 1.0, 4),
             (pose, z, neg_om, 1.0, 4), (pose, z, omega, np.nan, 4), (pose, z, omega, 0.0, 4), (pose, z, omega, -1.0, 4),
             (pose, z, omega, 1.0, 0), (pose, z, omega, 1.0, 9)]
    for case in cases:
        rc, outs = _raw(P, vals, *case)
        assert rc == ERR_INVALID, case
        assert all(np.all(o == 7) for o in outs), case
    rc, outs = _raw(P, vals, pose[:0], z[:0], None, 1.0, 4)                         # n_bearings == 0
    assert rc == bos.BOS_OK
    rc, outs = _raw(P, vals, pose, z, omega, np.inf, 8)
    assert rc == bos.BOS_OK and not any(np.any(o == 7) for o in outs[:5])
    lm, nis, count = expected_selection(outs[5][0], np.inf, 8)
    assert np.array_equal(outs[0][0], lm) and outs[4][0] == count == P.NL


def test_world_without_landmarks():
    """NL == 0: every count is 0 and every list is padding."""
    from helpers import chain_problem
    pose_xyt = np.array([[0.0, 0.0, 0.0], [1.0, 0.0, 0.1], [2.0, 0.2, 0.2], [3.0, 0.1, 0.3]])
    P = chain_problem(pose_xyt, 0, np.zeros(0, np.int32), np.zeros(0, np.int32), np.zeros(0))
    info = bos.plan_inspect(P, 0, 1, entries=True, solver=SCHUR)
    vals = np.where(info["rows"] == info["cols"], 10.0, 0.0)
    out = bos.plan_mf_associate_bearings(P, vals, [1, 3, 0], [0.1, 0.2, -4.0], k=3)
    assert np.all(out["cand_landmark"] == -1) and np.all(np.isinf(out["cand_nis"])) and np.all(out["n_inside"] == 0)
    assert np.all(out["cand_innovation"] == 0.0) and np.all(out["cand_var"] == 0.0) and out["nis_all"].shape == (3, 0)


def test_tile_constant():
    assert bos.associate_tile() >= 64 and bos.associate_tile() % 64 == 0
