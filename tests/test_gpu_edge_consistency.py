"""Solver.edge_consistency() (bos_edge_consistency: J+H build, multifrontal factorization, selected inverse with the
cross blocks' emission, projection kernel, scoring kernel, two selections) against tests/edge_consistency_ref.py at a
dense inverse of the system the same call linearised (export_system() right after it), against the host twin,
against edge_covariances() in its bits, for the selection's shapes, the NULL outputs, non-interference with the GN
steps around it, and the error paths."""
import ctypes

import numpy as np
import pytest

import bos
from conftest import MINI
from edge_consistency_ref import LIST_KEYS, ROW_KEYS, ConsistencyReference, check_lists
from helpers import gpu_lower
from test_edge_consistency_host import c1_world, check_duplicates, outlier_world, with_exact_duplicates
from test_edge_cov_host import edge_case_world

pytestmark = pytest.mark.gpu

SCHUR, SUPERNODAL = bos.BOS_SOLVER_SCHUR, bos.BOS_SOLVER_SUPERNODAL
ERR_INVALID = -1   # include/bos.h BOS_ERR_INVALID


@pytest.fixture(scope="module")
def c1():
    """C1 with the odometry's information divided by 100: both kinds of edges inside the reference's cap
    (test_edge_consistency_host.c1_world)."""
    return c1_world()


@pytest.fixture(scope="module")
def mini():
    return bos.load_g2o(MINI)


def _at(P, pose, lm):
    return bos.Problem(pose, lm, P.b_pose, P.b_lm, P.b_z, P.o_src, P.o_dst, P.o_z, P.o_omega, P.fixed, b_omega=P.b_omega,
                       pose_ids=P.pose_ids, lm_ids=P.lm_ids)


def _same(a, b, keys=LIST_KEYS + ROW_KEYS):
    return all(np.array_equal(a[k], b[k], equal_nan=True) for k in keys if a[k] is not None or b[k] is not None)


def _accuracy(P, S, what, trace=True, solver=SCHUR, schur_leaf=0):
    """The rows within the reference's bound with at most 1 % of either kind left out, the lists exactly, the trace
    identity (fp64 builds), bearing_redundancy from edge_covariances()' bearing_var in its bits, and the host twin on
    the call's own system within the same bound."""
    out = S.edge_consistency(k=8, rows=True)
    rows, cols, vals, _ = S.export_system()
    pose, lm = S.get_state()
    ref = ConsistencyReference(P, gpu_lower(rows, cols, vals, P.N), pose, lm)
    print(f"edge consistency gpu {what}:")
    assert out["solver_info"] == 0
    ref.check_rows(out, what)
    check_lists(out, 0.0, 0.0, 8)
    cov = S.edge_covariances(cross=False)
    om = 1.0 if P.b_omega is None else P.b_omega
    assert np.array_equal(out["bearing_redundancy"], 1.0 - om * cov["bearing_var"])
    if trace:
        ref.check_trace(out, 3 * (P.NP - 1) + 2 * P.NL, 0.01, cov["pose_cov"], cov["landmark_cov"], what)
    host = bos.plan_mf_edge_consistency(_at(P, pose, lm), vals, k=8, solver=solver, schur_leaf=schur_leaf)
    ref.check_rows(host, what + " (host twin)")
    loops = P.o_src == P.o_dst
    assert np.all(np.isnan(out["odom_w2"][loops])) and not set(np.nonzero(loops)[0]) & set(out["cand_odom"].tolist())
    return out


@pytest.mark.parametrize("solver", [SCHUR, SUPERNODAL])
def test_mini_dataset(mini, solver):
    """n = 18: M_b below one wavefront, both kinds inside the cap."""
    S = bos.Solver(mini, solver=solver)
    _accuracy(mini, S, f"mini solver {solver}", solver=solver)
    S.close()


@pytest.mark.parametrize("plan", ["schur", "supernodal", "schur_leaf40"])
def test_accuracy_fp64(c1, plan):
    kw = {"schur": dict(solver=SCHUR), "supernodal": dict(solver=SUPERNODAL), "schur_leaf40": dict(solver=SCHUR, schur_leaf=40)}[plan]
    S = bos.Solver(c1, **kw)
    _accuracy(c1, S, plan, **kw)
    S.close()


def test_accuracy_fp32(c1):
    """fp32 J+H, fp64 factor; e and J from the fp64 master state: against its own exported system."""
    S = bos.Solver(c1, precision=bos.BOS_FP32)
    _accuracy(c1, S, "fp32", trace=False)
    S.close()


def test_accuracy_after_steps(c1):
    """At the estimate of 10 GN iterations, the stream still busy with the last step when asked."""
    S = bos.Solver(c1)
    S.step_n(10)
    _accuracy(c1, S, "after 10 steps")
    S.close()


def test_edge_case_world(c1):
    """Duplicates, a reversed duplicate, self-loops, distant loop closures, bearings from the fixed pose: self-loops are
    NaN and never listed, duplicates of one orientation (their z redrawn) share the redundancy."""
    P = edge_case_world(c1)
    S = bos.Solver(P)
    out = _accuracy(P, S, "edge cases")
    S.close()
    assert (P.o_src == P.o_dst).sum() == 4
    seen, dups = {}, 0
    for e, key in enumerate(zip(P.b_pose.tolist(), P.b_lm.tolist())):
        f = seen.setdefault(key, e)
        if f != e:
            dups += 1
            assert out["bearing_redundancy"][e] == out["bearing_redundancy"][f]
    seen = {}
    for e, key in enumerate(zip(P.o_src.tolist(), P.o_dst.tolist())):
        f = seen.setdefault(key, e)
        if f != e and key[0] != key[1] and np.array_equal(P.o_omega[e], P.o_omega[f]):
            dups += 1
            assert out["odom_redundancy"][e] == out["odom_redundancy"][f]
    assert dups >= 40


def test_exact_duplicates_have_identical_bits(c1):
    """Bit-exact copies of the three worst bearings and odometry edges: rows, list entries, e and T in their bits."""
    S = bos.Solver(c1)
    first = S.edge_consistency(k=3)
    S.close()
    D, b_copy, o_copy = with_exact_duplicates(c1, first["cand_bearing"], first["cand_odom"])
    S = bos.Solver(D)
    out = S.edge_consistency(k=8, rows=True)
    S.close()
    assert out["solver_info"] == 0
    check_duplicates(out, first["cand_bearing"], b_copy, first["cand_odom"], o_copy)
    check_lists(out, 0.0, 0.0, 8)


def test_deterministic(c1):
    S = bos.Solver(c1)
    a = S.edge_consistency(k=8, rows=True)
    b = S.edge_consistency(k=8, rows=True)
    S.close()
    assert _same(a, b) and a["solver_info"] == b["solver_info"] == 0


def _with_extra_bearing(P):
    """P plus a copy of its first bearing: one edge more."""
    return bos.Problem(P.pose_xyt, P.lm_xy, np.append(P.b_pose, P.b_pose[0]), np.append(P.b_lm, P.b_lm[0]), np.append(P.b_z, P.b_z[0] + 0.01),
                       P.o_src, P.o_dst, P.o_z, P.o_omega, P.fixed)


def _without_odometry(P):
    return bos.Problem(P.pose_xyt, P.lm_xy, P.b_pose, P.b_lm, P.b_z, np.zeros(0, np.int32), np.zeros(0, np.int32), np.zeros((0, 3)),
                       np.zeros((0, 3, 3)), P.fixed)


@pytest.mark.parametrize("k", [1, 8])
@pytest.mark.parametrize("shape", ["below_a_wave", "one_tile", "one_tile_plus_1", "no_odometry"])
def test_selection_shapes(mini, shape, k):
    """The sizes at which the two-stage merge can go wrong: M_b below one wavefront, exactly one tile, one tile + 1 (a
    second tile of one edge), M_o = 0; gate 0, a gate that passes three, a gate above every score (all padding)."""
    tile = bos.associate_tile()
    P = {"below_a_wave": lambda: mini, "one_tile": lambda: bos.synthetic(tile // 8, 64, 8),
         "one_tile_plus_1": lambda: _with_extra_bearing(bos.synthetic(tile // 8, 64, 8)), "no_odometry": lambda: _without_odometry(mini)}[shape]()
    Mb = len(P.b_z)
    assert {"below_a_wave": Mb < 64, "one_tile": Mb == tile, "one_tile_plus_1": Mb == tile + 1, "no_odometry": len(P.o_z) == 0}[shape]
    S = bos.Solver(P)
    full = S.edge_consistency(k=k, rows=True)
    assert full["solver_info"] == 0
    rows = (full["bearing_w2"], full["odom_w2"])
    third = [float(np.sort(w[np.isfinite(w)])[-3]) if np.isfinite(w).sum() >= 3 else 0.0 for w in rows]
    above = [float(np.nanmax(w)) * 2 + 1 if np.isfinite(w).any() else 1.0 for w in rows]
    for gb, go in ((0.0, 0.0), tuple(third), tuple(above)):
        out = S.edge_consistency(gate_bearing=gb, gate_odom=go, k=k, rows=True)
        assert _same(out, full, ROW_KEYS)
        check_lists(out, gb, go, k)
    S.close()
    assert out["n_over_bearing"] == 0 and out["n_over_odom"] == 0 and np.all(out["cand_bearing"] == -1) and np.all(out["cand_odom"] == -1)
    assert np.all(np.isneginf(out["cand_bearing_w2"])) and np.all(out["cand_odom_rescov"] == 0.0)
    if shape == "no_odometry":
        assert full["n_over_odom"] == 0 and np.all(full["cand_odom"] == -1) and np.all(np.isneginf(full["cand_odom_w2"]))


def test_null_outputs(c1):
    """Lists only, rows only, one kind only, in every combination: what is returned has the full call's bits."""
    S = bos.Solver(c1)
    full = S.edge_consistency(k=4, rows=True)
    for lists in (True, False):
        for rows in (True, False):
            for kinds in (("bearing", "odom"), ("bearing",), ("odom",), ()):
                out = S.edge_consistency(k=4, rows=rows, lists=lists, kinds=kinds)
                assert out["solver_info"] == 0
                for key in LIST_KEYS + ROW_KEYS:
                    want = ("bearing" if "bearing" in key else "odom") in kinds and (lists if key in LIST_KEYS else rows)
                    assert (np.array_equal(out[key], full[key], equal_nan=True) if want else out[key] is None), (lists, rows, kinds, key)
    S.close()


def test_injected_outlier_is_listed_first(c1):
    """C1 converged, one bearing of its most observed landmark moved by 0.5 rad, converged again: the worst bearing."""
    P, edge = outlier_world(c1)
    S = bos.Solver(P)
    out = S.edge_consistency()
    S.close()
    assert out["solver_info"] == 0 and out["cand_bearing"][0] == edge


@pytest.mark.parametrize("precision", [bos.BOS_FP64, bos.BOS_FP32])
def test_steps_do_not_see_the_call(c1, precision):
    """The state is bit-identical across edge_consistency(); step, edge_consistency, step ends where step, step does."""
    A = bos.Solver(c1, precision=precision)
    B = bos.Solver(c1, precision=precision)
    A.step()
    B.step()
    before = A.get_state()
    A.edge_consistency(rows=True)
    after = A.get_state()
    assert np.array_equal(before[0], after[0]) and np.array_equal(before[1], after[1])
    sa = A.step()
    sb = B.step()
    pa, la = A.get_state()
    pb, lb = B.get_state()
    A.close()
    B.close()
    assert np.array_equal(pa, pb) and np.array_equal(la, lb)
    assert sa["chi2"] == sb["chi2"] and sa["solver_info"] == sb["solver_info"] == 0


@pytest.mark.parametrize("kind", ["dense", "rf"])
def test_unsupported_handles(mini, kind):
    kw = {"dense": dict(solver=bos.BOS_SOLVER_DENSE_CHOL), "rf": dict(solver=bos.BOS_SOLVER_ROCSOLVER_RF)}[kind]
    S = bos.Solver(mini, **kw)
    with pytest.raises(bos.BosError, match=r"\(-5\).*bos_edge_consistency"):
        S.edge_consistency()
    S.close()


def test_invalid_arguments_touch_nothing(mini):
    S = bos.Solver(mini)
    for gb, go, k in ((np.nan, 0.0, 4), (0.0, -1.0, 4), (np.inf, 0.0, 4), (0.0, 0.0, 0), (0.0, 0.0, 9)):
        out = bos._edge_check_arrays(mini, 8, True, True)
        for a in out.values():
            a.fill(7)
        info = ctypes.c_int32(7)
        rc = bos.lib().bos_edge_consistency(S._h, gb, go, k, *bos._edge_check_pointers(out), ctypes.byref(info))
        assert rc == ERR_INVALID and info.value == 7, (gb, go, k)
        assert all(np.all(a == 7) for a in out.values()), (gb, go, k)
    assert S.edge_consistency()["solver_info"] == 0      # the handle stays usable
    S.close()


def test_timing_getter(c1):
    S = bos.Solver(c1)
    assert S.edge_consistency_timing()["bytes"] == 0     # nothing is allocated before the first call
    S.edge_consistency()
    t = S.edge_consistency_timing()
    S.close()
    assert t["bytes"] > 0
    assert all(t[key] > 0.0 for key in ("host_ms", "jh_ms", "factor_ms", "selinv_ms", "score_ms", "select_ms", "download_ms"))
