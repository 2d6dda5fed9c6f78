"""Solver.match_landmarks() / Solver.match_poses() (bos_match_landmarks / bos_match_poses: J+H build,
multifrontal factorization, selected inverse, then per distinct query node the node column's projected slice,
the score kernel and the shared selection's two launches): the selection exactly against a stable sort of the
call's own rows with every listed score reproduced from its listed details, duplicates and ties, the rows
against tests/match_ref.py at the system the same call linearised and against the host twins, independence of
company, order and chunking, non-interference with the GN steps around the calls, NULL outputs and the error
paths."""
import ctypes

import numpy as np
import pytest

import bos
from conftest import C1, MINI
from helpers import EPS, gpu_lower
from marginals_ref import TOL_CAP, DenseInverses, sparse_tol
from match_ref import (CONDITION_CAP, LM_KEYS, POSE_KEYS, LandmarkReference, PoseReference, check_landmark_selection,
                       check_pose_selection, make_measurements, predicted_odometry, query_landmarks, query_poses, solve_rows)
from associate_ref import WRAP_GUARD, wrap
from test_gpu_node_cov import _pair_scales
from test_gpu_pair_cov import PLAN_KW

pytestmark = pytest.mark.gpu

ERR_INVALID = -1   # include/bos.h BOS_ERR_INVALID
LOWER = [0, 3, 4, 6, 7, 8]


@pytest.fixture(scope="module")
def c1():
    return bos.load_g2o(C1)


def _measurements(P, S, poses=None):
    return make_measurements(P, S.get_state()[0], query_poses(P) if poses is None else poses)


def _same(keys, x, y, rows_x=slice(None), rows_y=slice(None)):
    return all(np.array_equal(x[k][rows_x], y[k][rows_y], equal_nan=True) for k in keys)


# ---- 1. selection -------------------------------------------------------------------------------------------
_worlds = {}


def _world(name):
    """The selection tests' worlds, each generated once. three_tiles: three tiles of targets, the last one
    partial, their number no multiple of 64. The generator needs NP K >= 2 NL, and each landmark in front of
    every pose of its window of NP K / NL poses: 2 tile + 61 poses with 6 bearings each cannot be generated
    with 120 landmarks (windows of 105 poses; 960 is the least that can), so that world has 1200."""
    if name not in _worlds:
        N = 2 * bos.associate_tile() + 61
        _worlds[name] = {"mini": lambda: bos.load_g2o(MINI), "one_tile": lambda: bos.synthetic(60, 120, 6),
                         "three_tiles_lm": lambda: bos.synthetic(-(-2 * N // 12), N, 12),
                         "three_tiles_pose": lambda: bos.synthetic(N, 1200, 6)}[name]()
    return _worlds[name]


def _gates(rows, N):
    """+inf, one that passes a handful, one below every score."""
    return np.inf, float(np.sort(rows, axis=1)[:, min(4, N - 2)].max()), float(np.nanmin(rows)) / 2


@pytest.mark.parametrize("k", [1, 4, 8])
@pytest.mark.parametrize("name", ["mini", "one_tile", "three_tiles_lm"])
def test_landmark_selection_is_exact(name, k):
    P = _world(name)
    tile = bos.associate_tile()
    assert {"mini": P.NL < 8, "one_tile": 8 < P.NL < tile, "three_tiles_lm": 2 * tile < P.NL < 3 * tile and P.NL % 64}[name]
    S = bos.Solver(P)
    lms = np.array(query_landmarks(P), dtype=np.int32)
    full = S.match_landmarks(lms, k=k, d2_all=True)
    C = S.node_covariances(P.NP + lms, cross=False)["projected_landmark"]
    lm_xy = S.get_state()[1]
    rows = full["d2_all"]
    assert full["solver_info"] == 0 and np.all(full["n_inside"] == P.NL - 1)
    for gate in _gates(rows, P.NL):
        out = S.match_landmarks(lms, gate=gate, k=k, d2_all=True)
        assert out["solver_info"] == 0 and np.array_equal(out["d2_all"], rows, equal_nan=True)
        check_landmark_selection(out, gate, k)
        for q, a in enumerate(lms):
            assert np.isnan(rows[q, a]) and np.isfinite(np.delete(rows[q], a)).all()
            l = out["cand_landmark"][q][out["cand_landmark"][q] >= 0]
            assert np.array_equal(out["cand_cov"][q][:len(l)], C[q, l]), (q, gate)
            assert np.array_equal(out["cand_diff"][q][:len(l)], lm_xy[a] - lm_xy[l]), (q, gate)
    S.close()
    assert np.all(out["n_inside"] == 0) and np.all(out["cand_landmark"] == -1) and np.all(np.isinf(out["cand_d2"]))
    if name == "mini":
        assert k < 8 or np.all(full["cand_landmark"][:, P.NL - 1:] == -1)           # padding past the NL - 1 others


@pytest.mark.parametrize("k", [1, 4, 8])
@pytest.mark.parametrize("name", ["mini", "one_tile", "three_tiles_pose"])
def test_pose_selection_is_exact(name, k):
    P = _world(name)
    tile = bos.associate_tile()
    assert {"mini": P.NP < 8, "one_tile": 8 < P.NP < tile, "three_tiles_pose": 2 * tile < P.NP < 3 * tile and P.NP % 64}[name]
    S = bos.Solver(P)
    pose, z, omega = _measurements(P, S)
    full = S.match_poses(pose, z, omega, k=k, nis_all=True)
    distinct = sorted(set(pose.tolist()))
    Pm = S.node_covariances(distinct, cross=False)["projected_pose"]
    rows = full["nis_all"]
    assert full["solver_info"] == 0 and np.isfinite(rows).all() and np.all(full["n_inside"] == P.NP)
    for gate in _gates(rows, P.NP + 1):
        out = S.match_poses(pose, z, omega, gate=gate, k=k, nis_all=True)
        assert out["solver_info"] == 0 and np.array_equal(out["nis_all"], rows)
        check_pose_selection(out, gate, k)
        for q in range(len(pose)):
            u = out["cand_pose"][q][out["cand_pose"][q] >= 0]
            want = Pm[distinct.index(int(pose[q])), u] + bos.match_information_inverse(omega[q]).ravel()
            assert np.array_equal(out["cand_cov"][q][:len(u)][:, LOWER], want[:, LOWER]), (q, gate)
    S.close()
    assert np.all(out["n_inside"] == 0) and np.all(out["cand_pose"] == -1) and np.all(np.isinf(out["cand_nis"]))
    if name == "mini":
        assert k < 8 or np.all(full["cand_pose"][:, P.NP:] == -1)


# ---- 2. duplicates and ties ---------------------------------------------------------------------------------
def test_duplicates_and_ties():
    """Landmarks l1 < l2 moved onto l0's coordinates: both are listed first with d2 == 0.0, l1 before l2; l0
    itself is NaN, neither listed nor counted."""
    P = _world("one_tile")
    S = bos.Solver(P)
    pose_xyt, lm_xy = S.get_state()
    l0, l1, l2 = 40, 7, 93
    lm_xy[l1] = lm_xy[l0]
    lm_xy[l2] = lm_xy[l0]
    S.set_state(pose_xyt, lm_xy)
    out = S.match_landmarks([l0], gate=np.inf, k=8, d2_all=True)
    S.close()
    assert out["solver_info"] == 0
    check_landmark_selection(out, np.inf, 8)
    assert out["cand_landmark"][0][:2].tolist() == [l1, l2] and np.all(out["cand_d2"][0][:2] == 0.0)
    assert np.all(out["cand_diff"][0][:2] == 0.0) and np.all(out["cand_d2"][0][2:] > 0.0)
    assert np.isnan(out["d2_all"][0][l0]) and l0 not in out["cand_landmark"][0] and out["n_inside"][0] == P.NL - 1


# ---- 3. accuracy --------------------------------------------------------------------------------------------
_dense = {}


def _dense_of(P, Hl):
    """The dense inverses of one exported system, shared by the handles that export the same bits."""
    Hl = Hl.tocsr()
    Hl.sort_indices()
    key = (P.N, Hl.indptr.tobytes(), Hl.indices.tobytes(), Hl.data.tobytes())
    if key not in _dense:
        _dense[key] = DenseInverses(P, Hl)
    return _dense[key]


def _accuracy(P, S, what):
    lms = np.array(query_landmarks(P), dtype=np.int32)
    pose, z, omega = _measurements(P, S)
    lm_out = S.match_landmarks(lms, k=8, d2_all=True)
    pose_out = S.match_poses(pose, z, omega, k=8, nis_all=True)
    rows, cols, vals, _ = S.export_system()
    pose_xyt, lm_xy = S.get_state()
    Hl = gpu_lower(rows, cols, vals, P.N)
    dense = _dense_of(P, Hl)
    assert lm_out["solver_info"] == 0 and pose_out["solver_info"] == 0
    ref = LandmarkReference(P, Hl, lms, pose_xyt, lm_xy, dense=dense)
    ref.check_condition(f"gpu landmarks {what}")
    ref.check_scores(lm_out["d2_all"], f"gpu landmarks {what}")
    ref = PoseReference(P, Hl, pose, z, omega, pose_xyt, lm_xy, dense=dense)
    ref.check_condition(f"gpu poses {what}")
    ref.check_scores(pose_out["nis_all"], f"gpu poses {what}")
    check_landmark_selection(lm_out, np.inf, 8)
    check_pose_selection(pose_out, np.inf, 8)


@pytest.mark.parametrize("plan", ["schur", "supernodal", "schur_leaf40"])
def test_accuracy_fp64(c1, plan):
    S = bos.Solver(c1, **PLAN_KW[plan])
    _accuracy(c1, S, plan)
    S.close()


def test_accuracy_fp32(c1):
    """fp32 J+H, fp64 factor; d, e and the projection's J from the fp64 master state: against its own exported system."""
    S = bos.Solver(c1, precision=bos.BOS_FP32)
    _accuracy(c1, S, "fp32")
    S.close()


def test_accuracy_mini():
    P = _world("mini")
    S = bos.Solver(P)
    _accuracy(P, S, "mini")
    S.close()


# ---- 4. the host twins --------------------------------------------------------------------------------------
def _within_host_margin(gpu, host, M, v, tol_M, dv, keep, label):
    """|gpu - host| <= 2 |y|_1^2 tol_M + 4 |y|_1 dv + 64 eps host on the kept entries, y = M^-1 v from the
    host's own M; the condition tol_M |M^-1|_2 <= 0.1 first. Returns the worst share of the bound."""
    y, inv2 = solve_rows(M, v)
    y1 = np.abs(y).sum(axis=-1)
    with np.errstate(invalid="ignore"):
        lim = 2 * y1 ** 2 * tol_M + 4 * y1 * dv + 64 * EPS * host
        d = np.abs(gpu - host)
    assert float((tol_M * inv2)[keep].max()) <= CONDITION_CAP
    worst = float((d[keep] / np.maximum(lim[keep], 1e-300)).max())
    print(f"matching gpu vs host {label}: excluded {1 - keep.mean():.3g} worst |d| / bound {worst:.3g}")
    assert np.all(d[keep] <= lim[keep]), worst
    return worst


@pytest.mark.parametrize("which", ["c1", "one_tile"])
def test_gpu_matches_host(c1, which):
    """The host twins on the GPU's own exported values: the reference's bound with tol_M = 2 bound s_u s_v,
    bound = min(sparse tol, 1e-6) and s the projected entries' scales from the host's own diagonal blocks
    (test_gpu_node_cov.test_gpu_matches_host), M and the margins from the host's own blocks."""
    P = c1 if which == "c1" else _world("one_tile")
    S = bos.Solver(P)
    lms = np.array(query_landmarks(P), dtype=np.int32)
    pose, z, omega = _measurements(P, S)
    lm_out = S.match_landmarks(lms, k=8, d2_all=True)
    pose_out = S.match_poses(pose, z, omega, k=8, nis_all=True)
    rows, cols, vals, _ = S.export_system()
    S.close()
    assert lm_out["solver_info"] == 0 and pose_out["solver_info"] == 0
    tol, kappa = sparse_tol(P, gpu_lower(rows, cols, vals, P.N))
    bound = min(tol, TOL_CAP)
    distinct = sorted(set(pose.tolist()))
    node = bos.plan_mf_node_covariances(P, vals, list(P.NP + lms) + distinct)
    n_lm = len(lms)
    print(f"matching gpu vs host {which}: kappa_1 {kappa:.3g} tol {tol:.3g}")
    # landmarks
    host = bos.plan_mf_match_landmarks(P, vals, lms, k=8)
    a = np.repeat(P.NP + lms, P.NL)
    b = np.tile(P.NP + np.arange(P.NL, dtype=np.int32), n_lm)
    tol_M = 2 * bound * _pair_scales(P, a, b, node["pose_cov"], node["landmark_cov"])[1][:, :4].max(axis=1).reshape(n_lm, P.NL)
    M = node["projected_landmark"][:n_lm].reshape(n_lm, P.NL, 2, 2)
    v = P.lm_xy[lms][:, None, :] - P.lm_xy[None, :, :]
    dv = 64 * EPS * (np.linalg.norm(P.lm_xy[lms], axis=1)[:, None] + np.linalg.norm(P.lm_xy, axis=1)[None, :])
    keep = np.arange(P.NL)[None, :] != lms[:, None]
    _within_host_margin(lm_out["d2_all"], host["d2_all"], M, v, tol_M, dv, keep, f"{which} landmarks")
    check_landmark_selection(lm_out, np.inf, 8)
    # poses
    host = bos.plan_mf_match_poses(P, vals, pose, z, omega, k=8)
    a = np.repeat(np.array(distinct, dtype=np.int32), P.NP)
    b = np.tile(np.arange(P.NP, dtype=np.int32), len(distinct))
    row = np.array([distinct.index(int(p)) for p in pose])
    tol_M = 2 * bound * _pair_scales(P, a, b, node["pose_cov"], node["landmark_cov"])[1].max(axis=1).reshape(len(distinct), P.NP)[row]
    R = np.stack([bos.match_information_inverse(o) for o in omega])
    M = node["projected_pose"][n_lm:].reshape(len(distinct), P.NP, 3, 3)[row] + R[:, None, :, :]
    v = np.stack([predicted_odometry(P.pose_xyt, int(p)) for p in pose]) - z[:, None, :]
    v[:, :, 2] = wrap(v[:, :, 2])
    dist = np.linalg.norm(P.pose_xyt[None, :, :2] - P.pose_xyt[pose][:, None, :2], axis=2)
    dv = 64 * EPS * (1 + dist + np.linalg.norm(z, axis=1)[:, None])
    keep = np.abs(np.abs(v[:, :, 2]) - np.pi) > WRAP_GUARD
    assert 1 - keep.mean() <= 0.01
    _within_host_margin(pose_out["nis_all"], host["nis_all"], M, v, tol_M, dv, keep, f"{which} poses")
    check_pose_selection(pose_out, np.inf, 8)


# ---- 5. independence ----------------------------------------------------------------------------------------
def test_landmarks_independent_of_company_and_order(c1):
    """The same queries alone, reversed, beside other landmarks, with a repeated id and twice in a row:
    bit-identical per query."""
    P = c1
    S = bos.Solver(P)
    lms = np.array(query_landmarks(P) + [query_landmarks(P)[0], 5], dtype=np.int32)
    kw = dict(gate=50.0, k=4, d2_all=True)
    full = S.match_landmarks(lms, **kw)
    again = S.match_landmarks(lms, **kw)
    assert full["solver_info"] == 0 and _same(LM_KEYS, full, again)
    assert _same(LM_KEYS, S.match_landmarks(lms[::-1], **kw), full, slice(None), slice(None, None, -1))
    assert _same(LM_KEYS, full, full, slice(0, 1), slice(3, 4))                       # the repeated id
    for q in range(len(lms)):
        assert _same(LM_KEYS, S.match_landmarks(lms[q:q + 1], **kw), full, slice(None), slice(q, q + 1)), q
    for chunk in (1, 3, 0):
        S.debug_set_match_chunk(chunk)
        assert _same(LM_KEYS, S.match_landmarks(lms, **kw), full), chunk
    S.close()


def test_poses_independent_of_company_order_and_chunks(c1):
    """The same measurements alone, reversed, beside other poses' measurements, in chunks of 1 and 3, and
    twice in a row: bit-identical per measurement. The query poses include the fixed pose and the last one."""
    P = c1
    S = bos.Solver(P)
    pose, z, omega = _measurements(P, S)
    assert P.fixed in pose and P.NP - 1 in pose
    kw = dict(gate=50.0, k=4, nis_all=True)
    full = S.match_poses(pose, z, omega, **kw)
    again = S.match_poses(pose, z, omega, **kw)
    assert full["solver_info"] == 0 and _same(POSE_KEYS, full, again)
    rev = S.match_poses(pose[::-1], z[::-1], omega[::-1], **kw)
    assert _same(POSE_KEYS, rev, full, slice(None), slice(None, None, -1))
    for q0 in range(0, len(pose), 4):   # one pose's four measurements alone, then its second one alone
        alone = S.match_poses(pose[q0:q0 + 4], z[q0:q0 + 4], omega[q0:q0 + 4], **kw)
        assert _same(POSE_KEYS, alone, full, slice(None), slice(q0, q0 + 4)), q0
        one = S.match_poses(pose[q0 + 1:q0 + 2], z[q0 + 1:q0 + 2], omega[q0 + 1:q0 + 2], **kw)
        assert _same(POSE_KEYS, one, full, slice(None), slice(q0 + 1, q0 + 2)), q0
        assert _same(POSE_KEYS, full, full, slice(q0, q0 + 1), slice(q0 + 3, q0 + 4))   # the repeated entry
    for chunk in (1, 3, 0):
        S.debug_set_match_chunk(chunk)
        assert _same(POSE_KEYS, S.match_poses(pose, z, omega, **kw), full), chunk
    S.close()


# ---- 6. non-interference ------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", [bos.BOS_FP64, bos.BOS_FP32])
def test_steps_do_not_see_the_calls(c1, precision):
    """step_n(3), both calls, step_n(3) ends where step_n(6) does, bit for bit; bos_get_last_dx after a call
    is as after bos_marginals; the association on the same handle is not disturbed either."""
    A = bos.Solver(c1, precision=precision)
    B = bos.Solver(c1, precision=precision)
    A.step_n(3)
    before = A.get_state()
    pose, z, omega = _measurements(c1, A)
    assoc = A.associate_bearings([0, 5], [0.1, -0.2], gate=6.63, nis_all=True)
    assert A.match_landmarks(query_landmarks(c1), gate=9.21)["solver_info"] == 0
    with pytest.raises(bos.BosError, match=r"\(-1\)"):
        A.last_dx()
    assert A.match_poses(pose, z, omega, gate=11.34)["solver_info"] == 0
    with pytest.raises(bos.BosError, match=r"\(-1\)"):
        A.last_dx()
    after_assoc = A.associate_bearings([0, 5], [0.1, -0.2], gate=6.63, nis_all=True)
    assert all(np.array_equal(assoc[k], after_assoc[k]) for k in assoc)
    after = A.get_state()
    assert np.array_equal(before[0], after[0]) and np.array_equal(before[1], after[1])
    A.step_n(3)
    B.step_n(6)
    pa, la = A.get_state()
    pb, lb = B.get_state()
    A.close()
    B.close()
    assert np.array_equal(pa, pb) and np.array_equal(la, lb)


# ---- 7. NULL outputs and error paths ------------------------------------------------------------------------
def _raw(S, which, args, gate, k, mask=0x3f, fill=7):
    """The C call with sentinel-filled outputs, those of `mask` (bit i: the i-th output) passed, the rest
    NULL: (rc, outputs [.., 8 columns unless k is valid], solver_info)."""
    keys, dd, dc, N = (LM_KEYS, 2, 4, S.P.NL) if which == "landmarks" else (POSE_KEYS, 3, 9, S.P.NP)
    n, kk = len(args[0]), k if 1 <= k <= 8 else 8
    outs = [np.full((n, kk), fill, dtype=np.int32), np.full((n, kk), float(fill)), np.full((n, kk, dd), float(fill)),
            np.full((n, kk, dc), float(fill)), np.full(n, fill, dtype=np.int32), np.full((n, N), float(fill))]
    ins = [np.ascontiguousarray(args[0], dtype=np.int32)] + [None if x is None else np.ascontiguousarray(x, dtype=np.float64) for x in args[1:]]
    dp, ip = ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_int32)
    ptr = lambda x: None if x is None else x.ctypes.data_as(ip if x.dtype == np.int32 else dp)
    info = ctypes.c_int32(-99)
    f = bos.lib().bos_match_landmarks if which == "landmarks" else bos.lib().bos_match_poses
    rc = f(S._h, n, *[ptr(x) for x in ins], gate, k, *[ptr(o) if mask >> i & 1 else None for i, o in enumerate(outs)], ctypes.byref(info))
    return rc, dict(zip(keys, outs)), info.value


def test_null_outputs():
    """Every subset of the outputs: what is returned has the bits of the full call, what was not asked for is
    not written."""
    P = _world("one_tile")
    S = bos.Solver(P)
    lms = np.array(query_landmarks(P)[:2], dtype=np.int32)
    pose, z, omega = _measurements(P, S, [P.NP - 1])
    calls = {"landmarks": ((lms,), LM_KEYS, S.match_landmarks(lms, gate=50.0, k=4, d2_all=True)),
             "poses": ((pose, z, omega), POSE_KEYS, S.match_poses(pose, z, omega, gate=50.0, k=4, nis_all=True))}
    for which, (args, keys, full) in calls.items():
        for mask in range(64):
            rc, out, info = _raw(S, which, args, 50.0, 4, mask)
            assert rc == bos.BOS_OK and info == 0, (which, mask)
            for i, key in enumerate(keys):
                assert np.array_equal(out[key], full[key], equal_nan=True) if mask >> i & 1 else np.all(out[key] == 7), (which, mask, key)
    rc, out, _ = _raw(S, "poses", (pose, z, None), 50.0, 4)                           # omega NULL: the identity
    one = S.match_poses(pose, z, np.eye(3), gate=50.0, k=4, nis_all=True)
    assert rc == bos.BOS_OK and all(np.array_equal(out[k], one[k]) for k in POSE_KEYS)
    S.close()


def test_empty_calls_and_invalid_arguments(c1):
    P = c1
    S = bos.Solver(P)
    S.step()
    dx = S.last_dx()
    lms = np.array(query_landmarks(P), dtype=np.int32)
    pose, z, omega = _measurements(P, S)
    for which, args in (("landmarks", (lms[:0],)), ("poses", (pose[:0], z[:0], None))):
        rc, out, info = _raw(S, which, args, 1.0, 4)
        assert rc == bos.BOS_OK and info == -99                                         # n == 0 touches nothing
    bad_lm = lms.copy()
    bad_lm[1] = P.NL
    bad_pose, bad_z, nan_om, asym_om, neg_om = pose.copy(), z.copy(), omega.copy(), omega.copy(), omega.copy()
    bad_pose[1] = P.NP
    bad_z[2, 2] = np.nan
    nan_om[0, 8] = np.inf
    asym_om[1, 3] = np.nextafter(asym_om[1, 3], 1e9)
    neg_om[3] = np.diag([1.0, -1.0, 1.0]).ravel()
    cases = [("landmarks", (bad_lm,), 1.0, 4), ("landmarks", (-lms - 1,), 1.0, 4), ("landmarks", (lms,), np.nan, 4),
             ("landmarks", (lms,), 0.0, 4), ("landmarks", (lms,), -2.0, 4), ("landmarks", (lms,), 1.0, 0), ("landmarks", (lms,), 1.0, 9),
             ("poses", (bad_pose, z, omega), 1.0, 4), ("poses", (-pose - 1, z, omega), 1.0, 4), ("poses", (pose, bad_z, omega), 1.0, 4),
             ("poses", (pose, z, nan_om), 1.0, 4), ("poses", (pose, z, asym_om), 1.0, 4), ("poses", (pose, z, neg_om), 1.0, 4),
             ("poses", (pose, z, omega), np.nan, 4), ("poses", (pose, z, omega), 0.0, 4), ("poses", (pose, z, omega), -2.0, 4),
             ("poses", (pose, z, omega), 1.0, 0), ("poses", (pose, z, omega), 1.0, 9)]
    for case in cases:
        rc, out, info = _raw(S, *case)
        assert rc == ERR_INVALID and info == -99, case
        assert all(np.all(o == 7) for o in out.values()), case
    assert np.array_equal(S.last_dx(), dx)                                          # none of them linearised
    with pytest.raises(bos.BosError, match=r"\(-1\).*bos_match_landmarks"):
        S.match_landmarks([0], k=9)
    with pytest.raises(bos.BosError, match=r"\(-1\).*bos_match_poses"):
        S.match_poses([0], [[0.0, 0.0, 0.0]], k=0)
    S.close()


@pytest.mark.parametrize("kind", ["dense", "rf"])
def test_unsupported_handles(c1, kind):
    kw = {"dense": dict(solver=bos.BOS_SOLVER_DENSE_CHOL), "rf": dict(solver=bos.BOS_SOLVER_ROCSOLVER_RF)}[kind]
    S = bos.Solver(c1, **kw)
    with pytest.raises(bos.BosError, match=r"\(-5\).*bos_match_landmarks"):
        S.match_landmarks([0])
    with pytest.raises(bos.BosError, match=r"\(-5\).*bos_match_poses"):
        S.match_poses([0], [[0.0, 0.0, 0.0]])
    S.close()


# ---- 8. timing ----------------------------------------------------------------------------------------------
def test_timing(c1):
    S = bos.Solver(c1)
    assert S.match_timing()["match_bytes"] == 0                                     # nothing allocated before the first call
    pose, z, omega = _measurements(c1, S)
    for call in (lambda: S.match_landmarks(query_landmarks(c1), gate=9.21), lambda: S.match_poses(pose, z, omega, gate=11.34)):
        call()
        t = S.match_timing()
        assert t["match_bytes"] > 0
        assert all(np.isfinite(v) and v >= 0 for v in t.values())
        assert all(t[k] > 0 for k in ("jh_ms", "factor_ms", "selinv_ms", "column_ms", "score_ms", "select_ms"))
    S.close()
