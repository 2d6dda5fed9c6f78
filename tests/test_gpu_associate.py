"""Solver.associate_bearings() (bos_associate_bearings: J+H build, multifrontal factorization, selected
inverse, then per distinct pose the node column's projected_landmark, the NIS kernel and the two selection
launches): the selection exactly against a stable sort of the call's own rows, the rows against
tests/associate_ref.py at the system the same call linearised and against the host twin, independence of
company, order and chunking, non-interference with the GN steps around it, NULL outputs and the error
paths."""
import ctypes

import numpy as np
import pytest

import bos
from associate_ref import WRAP_GUARD, AssocReference, check_selection, make_bearings
from conftest import C1, MINI
from helpers import EPS, gpu_lower
from marginals_ref import TOL_CAP, DenseInverses, sparse_tol
from test_gpu_node_cov import _pair_scales
from test_gpu_pair_cov import PLAN_KW

pytestmark = pytest.mark.gpu

SCHUR = bos.BOS_SOLVER_SCHUR
OUT_KEYS = ("cand_landmark", "cand_nis", "cand_innovation", "cand_var", "n_inside", "nis_all")
ERR_INVALID = -1   # include/bos.h BOS_ERR_INVALID


@pytest.fixture(scope="module")
def c1():
    return bos.load_g2o(C1)


def _poses(P):
    """The fixed pose, the first, one in the middle and the last."""
    return sorted({P.fixed, 0, P.NP // 2, P.NP - 1})


def _bearings(P, S, poses=None):
    pose_xyt, lm_xy = S.get_state()
    return make_bearings(P, pose_xyt, lm_xy, _poses(P) if poses is None else poses)


def _same(x, y, rows_x=slice(None), rows_y=slice(None)):
    return all(np.array_equal(x[k][rows_x], y[k][rows_y]) for k in OUT_KEYS)


# ---- 1. selection -------------------------------------------------------------------------------------------
_worlds = {}


def _world(name):
    """The selection tests' worlds, each generated once."""
    if name not in _worlds:
        if name == "mini":
            P = bos.load_g2o(MINI)
        elif name == "one_tile":
            P = bos.synthetic(60, 120, 6)
        else:   # three tiles, the last one partial, NL no multiple of 64; the generator needs NP K >= 2 NL
            NL = 2 * bos.associate_tile() + 61
            P = bos.synthetic(-(-2 * NL // 12), NL, 12)
        _worlds[name] = P
    return _worlds[name]


@pytest.mark.parametrize("k", [1, 4, 8])
@pytest.mark.parametrize("name", ["mini", "one_tile", "three_tiles"])
def test_selection_is_exact(name, k):
    """Gates +inf, one that passes a handful of landmarks, one below every NIS (all counts 0, all padding);
    MINI has NL < 8 (padding at k = 8), the synthetic worlds one tile and three."""
    P = _world(name)
    tile = bos.associate_tile()
    assert {"mini": P.NL < 8, "one_tile": 8 < P.NL < tile, "three_tiles": 2 * tile < P.NL < 3 * tile and P.NL % 64}[name]
    S = bos.Solver(P)
    pose, z, omega = _bearings(P, S)
    full = S.associate_bearings(pose, z, omega, k=k, nis_all=True)
    distinct = sorted(set(pose.tolist()))
    var = S.node_covariances(distinct, cross=False)["projected_landmark"][:, :, 0]
    rows = full["nis_all"]
    assert full["solver_info"] == 0 and np.isfinite(rows).all()
    handful = float(np.sort(rows, axis=1)[:, min(4, P.NL - 1)].max())
    for gate in (np.inf, handful, float(rows.min()) / 2):
        out = S.associate_bearings(pose, z, omega, gate=gate, k=k, nis_all=True)
        assert out["solver_info"] == 0 and np.array_equal(out["nis_all"], rows)
        check_selection(out, gate, k)
        for q in range(len(pose)):
            listed = out["cand_landmark"][q] >= 0
            v = var[distinct.index(int(pose[q])), out["cand_landmark"][q][listed]]
            assert np.array_equal(out["cand_var"][q][listed], v + 1 / omega[q]), (q, gate)
    S.close()
    assert np.all(out["n_inside"] == 0) and np.all(out["cand_landmark"] == -1) and np.all(np.isinf(out["cand_nis"]))
    assert np.all(full["n_inside"] == P.NL)


def test_ties_go_to_the_lower_stix():
    """Two landmarks with identical coordinates: their e has equal bits, their NIS need not. Wherever two
    listed entries carry equal NIS bits the lower stix comes first; the list is ascending throughout."""
    P = _world("one_tile")
    S = bos.Solver(P)
    pose_xyt, lm_xy = S.get_state()
    a = 0 if P.fixed != 0 else 1
    l0 = int(P.b_lm[P.b_pose == a][0])
    l1 = (l0 + 1) % P.NL
    lm_xy[l1] = lm_xy[l0]
    S.set_state(pose_xyt, lm_xy)
    pose, z, omega = make_bearings(P, pose_xyt, lm_xy, [a, P.fixed])
    out = S.associate_bearings(pose, z, omega, gate=np.inf, k=8, nis_all=True)
    S.close()
    assert out["solver_info"] == 0
    check_selection(out, np.inf, 8)
    for q in range(len(pose)):
        nis, lm = out["cand_nis"][q], out["cand_landmark"][q]
        for j in range(7):
            assert nis[j] < nis[j + 1] or (nis[j] == nis[j + 1] and lm[j] < lm[j + 1]), (q, j)
    q = 0   # the first bearing aims at l0: both copies are listed, with one innovation
    both = [int(np.nonzero(out["cand_landmark"][q] == l)[0][0]) for l in (l0, l1)]
    assert out["cand_innovation"][q][both[0]] == out["cand_innovation"][q][both[1]]


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
    pose, z, omega = _bearings(P, S)
    out = S.associate_bearings(pose, z, omega, k=8, nis_all=True)
    rows, cols, vals, _ = S.export_system()
    pose_xyt, lm_xy = S.get_state()
    Hl = gpu_lower(rows, cols, vals, P.N)
    ref = AssocReference(P, Hl, pose, z, omega, pose_xyt, lm_xy, dense=_dense_of(P, Hl))
    assert out["solver_info"] == 0
    ref.check_nis(out["nis_all"], f"gpu {what}")
    check_selection(out, np.inf, 8)


@pytest.mark.parametrize("plan", ["schur", "supernodal", "schur_leaf40"])
def test_accuracy_fp64(c1, plan):
    S = bos.Solver(c1, **PLAN_KW[plan])
    _accuracy(c1, S, plan)
    S.close()


def test_accuracy_fp32(c1):
    """fp32 J+H, fp64 factor; e and the projection's J from the fp64 master state: against its own exported system."""
    S = bos.Solver(c1, precision=bos.BOS_FP32)
    _accuracy(c1, S, "fp32")
    S.close()


# ---- 4. the host twin ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["c1", "c2"])
def test_gpu_matches_host(c1, which):
    """The host twin on the GPU's own exported values: the rows within nis (2 bound s^2 / S + 64 eps), bound =
    min(sparse tol, 1e-6) and s^2 the projected entry's scale of test_gpu_node_cov.test_gpu_matches_host
    (from the host's own diagonal blocks), S the host's. Config 2 (synthetic 1000 / 2000 / 20) has fronts
    of 65-128 rows."""
    P = c1 if which == "c1" else bos.synthetic(1000, 2000, 20)
    S = bos.Solver(P)
    pose, z, omega = _bearings(P, S, None if which == "c1" else [P.fixed, P.NP - 1])
    out = S.associate_bearings(pose, z, omega, k=8, nis_all=True)
    rows, cols, vals, _ = S.export_system()
    S.close()
    assert out["solver_info"] == 0
    host = bos.plan_mf_associate_bearings(P, vals, pose, z, omega, k=8)
    distinct = sorted(set(pose.tolist()))
    node = bos.plan_mf_node_covariances(P, vals, distinct, solver=SCHUR)
    tol, kappa = sparse_tol(P, gpu_lower(rows, cols, vals, P.N))
    bound = min(tol, TOL_CAP)
    a = np.repeat(np.array(distinct, dtype=np.int32), P.NL)
    b = np.tile(P.NP + np.arange(P.NL, dtype=np.int32), len(distinct))
    s2 = _pair_scales(P, a, b, node["pose_cov"], node["landmark_cov"])[1][:, 0].reshape(len(distinct), P.NL)
    row = np.array([distinct.index(int(p)) for p in pose])
    S_h = node["projected_landmark"][row, :, 0] + (1 / omega)[:, None]
    lim = host["nis_all"] * (2 * bound * s2[row] / S_h + 64 * EPS)
    d = np.abs(out["nis_all"] - host["nis_all"])
    # the innovation at the wrap flips on a last-ulp difference of the two cos / sin; found from the host's list
    e_h = np.sqrt(host["nis_all"] * S_h)
    keep = np.abs(e_h - np.pi) > WRAP_GUARD
    worst = float((d[keep] / np.maximum(lim[keep], 1e-300)).max())
    print(f"association gpu vs host {which}: kappa_1 {kappa:.3g} tol {tol:.3g} excluded {1 - keep.mean():.3g} worst |d| / bound {worst:.3g}")
    assert 1 - keep.mean() <= 0.01
    assert np.all(d[keep] <= lim[keep])
    check_selection(out, np.inf, 8)


# ---- 5. independence ----------------------------------------------------------------------------------------
def test_independent_of_company_order_and_chunks(c1):
    """The same bearings alone, reversed, beside other poses' bearings, in chunks of 1 and 3, and twice in a
    row: bit-identical per bearing. The query poses include the fixed pose and the last one."""
    P = c1
    S = bos.Solver(P)
    pose, z, omega = _bearings(P, S)
    assert P.fixed in pose and P.NP - 1 in pose
    kw = dict(gate=20.0, k=4, nis_all=True)
    full = S.associate_bearings(pose, z, omega, **kw)
    again = S.associate_bearings(pose, z, omega, **kw)
    assert full["solver_info"] == 0 and _same(full, again)
    n = len(pose)
    rev = S.associate_bearings(pose[::-1], z[::-1], omega[::-1], **kw)
    assert _same(rev, full, slice(None), slice(None, None, -1))
    for q0 in range(0, n, 4):   # one pose's four bearings alone, then its second bearing alone
        alone = S.associate_bearings(pose[q0:q0 + 4], z[q0:q0 + 4], omega[q0:q0 + 4], **kw)
        assert _same(alone, full, slice(None), slice(q0, q0 + 4)), q0
        one = S.associate_bearings(pose[q0 + 1:q0 + 2], z[q0 + 1:q0 + 2], omega[q0 + 1:q0 + 2], **kw)
        assert _same(one, full, slice(None), slice(q0 + 1, q0 + 2)), q0
        assert _same(full, full, slice(q0, q0 + 1), slice(q0 + 3, q0 + 4))            # the repeated entry
    for chunk in (1, 3, 0):
        S.debug_set_associate_chunk(chunk)
        assert _same(S.associate_bearings(pose, z, omega, **kw), full), chunk
    S.close()


# ---- 6. non-interference ------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", [bos.BOS_FP64, bos.BOS_FP32])
def test_steps_do_not_see_the_call(c1, precision):
    """step_n(3), associate, step_n(3) ends where step_n(6) does, bit for bit; bos_get_last_dx after the
    call is as after bos_marginals."""
    A = bos.Solver(c1, precision=precision)
    B = bos.Solver(c1, precision=precision)
    A.step_n(3)
    before = A.get_state()
    pose, z, omega = _bearings(c1, A)
    out = A.associate_bearings(pose, z, omega, gate=6.63, nis_all=True)
    assert out["solver_info"] == 0
    with pytest.raises(bos.BosError, match=r"\(-1\)"):
        A.last_dx()
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
def _raw(S, pose, z, omega, gate, k, mask=0x3f, fill=7):
    """The C call with sentinel-filled outputs, those of `mask` (bit i: OUT_KEYS[i]) passed, the rest NULL:
    (rc, outputs [.., 8 columns], solver_info)."""
    n, NL = len(pose), S.P.NL
    a, zz = np.ascontiguousarray(pose, dtype=np.int32), np.ascontiguousarray(z, dtype=np.float64)
    om = None if omega is None else np.ascontiguousarray(omega, dtype=np.float64)
    outs = [np.full((n, k if 1 <= k <= 8 else 8), fill, dtype=np.int32)] + [np.full((n, k if 1 <= k <= 8 else 8), float(fill)) for _ in range(3)]
    outs += [np.full(n, fill, dtype=np.int32), np.full((n, NL), float(fill))]
    dp, ip = ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_int32)
    ptr = lambda x: None if x is None else x.ctypes.data_as(ip if x.dtype == np.int32 else dp)
    info = ctypes.c_int32(-99)
    rc = bos.lib().bos_associate_bearings(S._h, n, ptr(a), ptr(zz), ptr(om), gate, k,
                                          *[ptr(o) if mask >> i & 1 else None for i, o in enumerate(outs)], ctypes.byref(info))
    return rc, dict(zip(OUT_KEYS, outs)), info.value


def test_null_outputs(c1):
    """Every single output alone, none and all: what is returned has the bits of the full call, what was
    not asked for is not written."""
    S = bos.Solver(c1)
    pose, z, omega = _bearings(c1, S)
    full = S.associate_bearings(pose, z, omega, gate=20.0, k=4, nis_all=True)
    for mask in [0, 0x3f, 0x1f] + [1 << i for i in range(6)]:
        rc, out, info = _raw(S, pose, z, omega, 20.0, 4, mask)
        assert rc == bos.BOS_OK and info == 0, mask
        for i, key in enumerate(OUT_KEYS):
            assert np.array_equal(out[key], full[key]) if mask >> i & 1 else np.all(out[key] == 7), (mask, key)
    rc, out, _ = _raw(S, pose, z, None, 20.0, 4)                                    # omega NULL: 1
    one = S.associate_bearings(pose, z, np.ones(len(pose)), gate=20.0, k=4, nis_all=True)
    assert rc == bos.BOS_OK and all(np.array_equal(out[k], one[k]) for k in OUT_KEYS)
    S.close()


def test_empty_call_and_invalid_arguments(c1):
    P = c1
    S = bos.Solver(P)
    S.step()
    dx = S.last_dx()
    pose, z, omega = _bearings(P, S)
    rc, out, info = _raw(S, pose[:0], z[:0], None, 1.0, 4)
    assert rc == bos.BOS_OK and info == -99                                         # n_bearings == 0 touches nothing
    bad_pose, bad_z, bad_om, zero_om = pose.copy(), z.copy(), omega.copy(), omega.copy()
    bad_pose[1] = P.NP
    bad_z[2] = np.nan
    bad_om[0] = np.inf
    zero_om[3] = 0.0
    cases = [(bad_pose, z, omega, 1.0, 4), (-pose - 1, z, omega, 1.0, 4), (pose, bad_z, omega, 1.0, 4), (pose, z, bad_om, 1.0, 4),
             (pose, z, zero_om, 1.0, 4), (pose, z, omega, np.nan, 4), (pose, z, omega, 0.0, 4), (pose, z, omega, -2.0, 4),
             (pose, z, omega, 1.0, 0), (pose, z, omega, 1.0, 9)]
    for case in cases:
        rc, out, info = _raw(S, *case)
        assert rc == ERR_INVALID and info == -99, case
        assert all(np.all(o == 7) for o in out.values()), case
    assert np.array_equal(S.last_dx(), dx)                                          # none of them linearised
    with pytest.raises(bos.BosError, match=r"\(-1\).*bos_associate_bearings"):
        S.associate_bearings([0], [0.0], k=9)
    S.close()


@pytest.mark.parametrize("kind", ["dense", "rf", "communicator"])
def test_unsupported_handles(c1, kind):
    kw = {"dense": dict(solver=bos.BOS_SOLVER_DENSE_CHOL), "rf": dict(solver=bos.BOS_SOLVER_ROCSOLVER_RF),
          "communicator": dict(solver=SCHUR, rank=0, world_size=1, nccl_id=bos.nccl_unique_id())}[kind]
    S = bos.Solver(c1, **kw)
    with pytest.raises(bos.BosError, match=r"\(-5\).*bos_associate_bearings"):
        S.associate_bearings([0], [0.0])
    S.close()


# ---- 8. timing ----------------------------------------------------------------------------------------------
def test_timing(c1):
    S = bos.Solver(c1)
    assert S.associate_bearings_timing()["assoc_bytes"] == 0                        # nothing allocated before the first call
    pose, z, omega = _bearings(c1, S)
    S.associate_bearings(pose, z, omega, gate=6.63)
    t = S.associate_bearings_timing()
    S.close()
    assert t["assoc_bytes"] > 0
    assert all(np.isfinite(v) and v >= 0 for v in t.values())
    assert all(t[k] > 0 for k in ("jh_ms", "factor_ms", "selinv_ms", "column_ms", "nis_ms", "select_ms"))
