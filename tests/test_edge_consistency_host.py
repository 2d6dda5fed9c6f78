"""Edge consistency on the host (bos_plan_mf_edge_consistency: bearing_var / odom_cov of the host selected inverse,
then e, T, w2, chi2 and the redundancy by csrc/host/edge_check.hpp and a plain stable sort) against
tests/edge_consistency_ref.py at a dense inverse of the oracle's H_nf: the rows within the reference's bound, the
trace identity, the lists exactly against the twin's own rows, an injected outlier, and the argument rules."""
import ctypes

import numpy as np
import pytest

import bos
import oracle as O
from conftest import C1, MINI
from edge_consistency_ref import LIST_KEYS, ROW_KEYS, ConsistencyReference, check_lists, expected_list
from helpers import oracle_lower_nf, to_oracle
from test_edge_cov_host import edge_case_world

SCHUR, SUPERNODAL = bos.BOS_SOLVER_SCHUR, bos.BOS_SOLVER_SUPERNODAL
ERR_INVALID = -1   # include/bos.h BOS_ERR_INVALID
DAMPING = 0.01


def one_pose_world(seed=5):
    """The fixed pose alone with 6 landmarks, each seen three times from it: M_o = 0, every cross block zero."""
    rng = np.random.default_rng(seed)
    pose = np.array([[0.3, -0.2, 0.4]])
    lm = pose[0, :2] + rng.uniform(2.0, 6.0, (6, 1)) * np.stack([np.cos(a := rng.uniform(-3, 3, 6)), np.sin(a)], axis=1)
    b_lm = np.repeat(np.arange(6, dtype=np.int32), 3)
    z = np.array([O.predict_bearing(pose[0], lm[l]) for l in b_lm]) + rng.normal(0, 0.02, len(b_lm))
    return bos.Problem(pose, lm + rng.normal(0, 0.05, lm.shape), np.zeros(len(b_lm), dtype=np.int32), b_lm, z,
                       np.zeros(0, np.int32), np.zeros(0, np.int32), np.zeros((0, 3)), np.zeros((0, 3, 3)), 0)


def soft_odometry_world(P, factor=100.0):
    """P with the odometry's information divided by `factor`. On the datasets themselves an odometry edge has a
    redundancy of about 0.01 and the reference's own error swallows T for most of them (edge_consistency_ref.py:
    the cap on excluded entries is not met); here it is about 0.14 and no odometry edge is excluded."""
    return bos.Problem(P.pose_xyt, P.lm_xy, P.b_pose, P.b_lm, P.b_z, P.o_src, P.o_dst, P.o_z, P.o_omega / factor, P.fixed,
                       b_omega=P.b_omega, pose_ids=P.pose_ids, lm_ids=P.lm_ids)


def c1_world():
    """The C1 of the accuracy tests: the dataset with its odometry's information divided by 100, so that both kinds
    of edges stay inside the reference's cap on excluded entries."""
    return soft_odometry_world(bos.load_g2o(C1))


def with_exact_duplicates(P, bearings, odometry):
    """P plus bit-exact copies (z and information included) of the given bearings and odometry edges, appended in
    that order: (problem, indices of the bearing copies, indices of the odometry copies). The first of the odometry
    edges has its measurement moved by (0.3, -0.2, 0.1) before it is copied: a duplicated odometry edge loses
    half its weight in w2, and this one has to stay the worst so that it and its copy are listed."""
    b, o = np.asarray(bearings, dtype=np.int64), np.asarray(odometry, dtype=np.int64)
    o_z = P.o_z.copy()
    o_z[o[0]] += np.array([0.3, -0.2, 0.1])
    P = bos.Problem(P.pose_xyt, P.lm_xy, P.b_pose, P.b_lm, P.b_z, P.o_src, P.o_dst, o_z, P.o_omega, P.fixed, b_omega=P.b_omega)
    Q = bos.Problem(P.pose_xyt, P.lm_xy, np.append(P.b_pose, P.b_pose[b]), np.append(P.b_lm, P.b_lm[b]), np.append(P.b_z, P.b_z[b]),
                    np.append(P.o_src, P.o_src[o]), np.append(P.o_dst, P.o_dst[o]), np.concatenate([P.o_z, P.o_z[o]]),
                    np.concatenate([P.o_omega, P.o_omega[o]]), P.fixed,
                    b_omega=None if P.b_omega is None else np.append(P.b_omega, P.b_omega[b]))
    return Q, len(P.b_z) + np.arange(len(b)), len(P.o_z) + np.arange(len(o))


def check_duplicates(out, bearings, b_copy, odometry, o_copy):
    """An exact copy of an edge has the original's w2, chi2 and redundancy in their bits, is listed right behind it
    when the original is listed (equal w2 go to the lower index first), and then with the same e and T."""
    for kind, orig, copy in (("bearing", bearings, b_copy), ("odom", odometry, o_copy)):
        for key in ("w2", "chi2", "redundancy"):
            assert np.array_equal(out[f"{kind}_{key}"][orig], out[f"{kind}_{key}"][copy]), (kind, key)
        cand = out[f"cand_{kind}"].tolist()
        T = out["cand_bearing_resvar" if kind == "bearing" else "cand_odom_rescov"]
        both = 0
        for a, c in zip(orig, copy):
            if a in cand and cand.index(a) + 1 < len(cand):
                j = cand.index(a)
                assert cand[j + 1] == c, (kind, cand, a, c)
                assert np.array_equal(out[f"cand_{kind}_innovation"][j], out[f"cand_{kind}_innovation"][j + 1])
                assert np.array_equal(T[j], T[j + 1]) and out[f"cand_{kind}_w2"][j] == out[f"cand_{kind}_w2"][j + 1]
                both += 1
        assert both >= 1, kind


_cache = {}


def _case(which):
    """Problem, the oracle's lower H_nf and the reference: once per world."""
    if which not in _cache:
        if which == "one_pose":
            P = one_pose_world()
        else:
            P = bos.load_g2o(MINI) if which == "mini" else c1_world()
            if which == "edge_cases":
                P = edge_case_world(P)
            if which == "c1_converged":
                P = converged(P)
        Q = to_oracle(P)
        Hl = oracle_lower_nf(Q, O.linearize(Q, damping=DAMPING)).tocsr()
        _cache[which] = (P, Hl, ConsistencyReference(P, Hl))
    return _cache[which]


def _vals(P, Hl, solver, leaf):
    info = bos.plan_inspect(P, 0, 1, entries=True, solver=solver, schur_leaf=leaf)
    return np.asarray(Hl[info["rows"], info["cols"]]).ravel()


PLANS = [("mini", SCHUR, 0), ("mini", SUPERNODAL, 0), ("c1", SCHUR, 0), ("c1", SUPERNODAL, 0), ("c1", SCHUR, 40),
         ("c1_converged", SCHUR, 0), ("edge_cases", SCHUR, 0), ("edge_cases", SUPERNODAL, 0), ("one_pose", SCHUR, 0)]


@pytest.mark.parametrize("which,solver,leaf", PLANS)
def test_rows_against_reference(which, solver, leaf):
    """w2 within the reference's first-order bound with at most 1 % of either kind left out, chi2, the NaN rule of
    self-loops, the redundancy's range, and the trace identity sum tr(Omega P) = n - lambda tr(Sigma)."""
    P, Hl, ref = _case(which)
    vals = _vals(P, Hl, solver, leaf)
    out = bos.plan_mf_edge_consistency(P, vals, k=8, solver=solver, schur_leaf=leaf)
    label = f"host {which} solver {solver} leaf {leaf}"
    ref.check_rows(out, label)
    pose_cov, lm_cov = bos.plan_mf_marginals(P, vals, solver=solver, schur_leaf=leaf)
    ref.check_trace(out, 3 * (P.NP - 1) + 2 * P.NL, DAMPING, pose_cov, lm_cov, label)
    check_lists(out, 0.0, 0.0, 8)
    cov = bos.plan_mf_edge_covariances(P, vals, solver=solver, schur_leaf=leaf)
    om = 1.0 if P.b_omega is None else P.b_omega
    assert np.array_equal(out["bearing_redundancy"], 1.0 - om * cov["bearing_var"])


def test_edge_case_world_rules():
    """Self-loops are NaN and never listed; duplicates of one orientation (their z redrawn) share the redundancy."""
    P, Hl, _ = _case("edge_cases")
    out = bos.plan_mf_edge_consistency(P, _vals(P, Hl, SCHUR, 0), k=8)
    loops = np.nonzero(P.o_src == P.o_dst)[0]
    assert len(loops) == 4 and not set(loops) & set(out["cand_odom"].tolist())
    assert np.all(np.isnan(out["odom_w2"][loops])) and np.all(np.isfinite(out["odom_chi2"][loops]))
    assert out["n_over_odom"] == np.isfinite(out["odom_w2"]).sum()
    seen, dups = {}, 0
    for e, key in enumerate(zip(P.b_pose.tolist(), P.b_lm.tolist())):
        f = seen.setdefault(key, e)
        if f != e:
            dups += 1
            assert out["bearing_redundancy"][e] == out["bearing_redundancy"][f]
            if P.b_z[e] == P.b_z[f]:
                assert out["bearing_w2"][e] == out["bearing_w2"][f]
    seen = {}
    for e, key in enumerate(zip(P.o_src.tolist(), P.o_dst.tolist())):
        f = seen.setdefault(key, e)
        if f != e and np.array_equal(P.o_omega[e], P.o_omega[f]):
            dups += 1
            assert out["odom_redundancy"][e] == out["odom_redundancy"][f] or key[0] == key[1]
    assert dups >= 40


@pytest.mark.parametrize("k", [1, 4, 8])
@pytest.mark.parametrize("which", ["mini", "c1", "one_pose"])
def test_lists_are_exact(which, k):
    """Gate 0, a gate that passes a handful, a gate above every score (all padding, counts 0)."""
    P, Hl, _ = _case(which)
    vals = _vals(P, Hl, SCHUR, 0)
    full = bos.plan_mf_edge_consistency(P, vals, k=k)
    tops = [float(np.sort(w[np.isfinite(w)])[-3]) if np.isfinite(w).sum() >= 3 else 0.0 for w in (full["bearing_w2"], full["odom_w2"])]
    above = [float(np.nanmax(w)) * 2 + 1 if len(w) else 1.0 for w in (full["bearing_w2"], full["odom_w2"])]
    for gb, go in ((0.0, 0.0), tuple(tops), tuple(above)):
        out = bos.plan_mf_edge_consistency(P, vals, gate_bearing=gb, gate_odom=go, k=k)
        assert all(np.array_equal(out[r], full[r], equal_nan=True) for r in ROW_KEYS)
        check_lists(out, gb, go, k)
    assert out["n_over_bearing"] == 0 and out["n_over_odom"] == 0 and np.all(out["cand_bearing"] == -1) and np.all(out["cand_odom"] == -1)
    assert np.all(np.isneginf(out["cand_bearing_w2"])) and np.all(np.isneginf(out["cand_odom_w2"]))
    if which == "one_pose":
        assert len(full["odom_w2"]) == 0 and full["n_over_odom"] == 0 and np.all(full["cand_odom"] == -1)


def converged(P, iterations=12):
    """P at the estimate of `iterations` CPU Gauss-Newton steps."""
    G = bos.CpuGN(P, 4)
    for _ in range(iterations):
        G.step()
    pose, lm = G.get_state()
    G.close()
    return bos.Problem(pose, lm, P.b_pose, P.b_lm, P.b_z, P.o_src, P.o_dst, P.o_z, P.o_omega, P.fixed, b_omega=P.b_omega,
                       pose_ids=P.pose_ids, lm_ids=P.lm_ids)


def test_exact_duplicates_have_identical_bits():
    """Bit-exact copies of the three worst bearings and odometry edges: rows, list entries, e and T in their bits."""
    P, Hl, _ = _case("c1")
    first = bos.plan_mf_edge_consistency(P, _vals(P, Hl, SCHUR, 0), k=3, rows=False)
    D, b_copy, o_copy = with_exact_duplicates(P, first["cand_bearing"], first["cand_odom"])
    Q = to_oracle(D)
    Hd = oracle_lower_nf(Q, O.linearize(Q, damping=DAMPING)).tocsr()
    out = bos.plan_mf_edge_consistency(D, _vals(D, Hd, SCHUR, 0), k=8)
    check_duplicates(out, first["cand_bearing"], b_copy, first["cand_odom"], o_copy)
    check_lists(out, 0.0, 0.0, 8)


def outlier_world(P0, shift=0.5):
    """(problem, edge): P0 converged, the first bearing of its most observed landmark shifted by `shift` rad,
    converged again."""
    A = converged(P0)
    l = int(np.argmax(np.bincount(A.b_lm, minlength=A.NL)))
    edge = int(np.nonzero(A.b_lm == l)[0][0])
    z = A.b_z.copy()
    z[edge] = z[edge] + shift
    B = bos.Problem(A.pose_xyt, A.lm_xy, A.b_pose, A.b_lm, z, A.o_src, A.o_dst, A.o_z, A.o_omega, A.fixed, b_omega=A.b_omega,
                    pose_ids=A.pose_ids, lm_ids=A.lm_ids)
    return converged(B), edge


def test_injected_outlier_is_found():
    """A bearing of a well-observed landmark moved by 0.5 rad is the worst bearing in the reference and in the twin."""
    P, edge = outlier_world(c1_world())
    Q = to_oracle(P)
    Hl = oracle_lower_nf(Q, O.linearize(Q, damping=DAMPING)).tocsr()
    ref = ConsistencyReference(P, Hl)
    rank = np.argsort(-np.where(ref.b_keep, ref.b_w2, -np.inf), kind="stable")
    print(f"  injected outlier: edge {edge} w2_ref {ref.b_w2[edge]:.4g}, next {ref.b_w2[rank[1]]:.4g}")
    assert rank[0] == edge and ref.b_keep[edge]
    # the datasets' bearings carry the information 1 (a standard deviation of 1 rad): 0.5 rad is the worst, below any
    # chi^2 gate
    out = bos.plan_mf_edge_consistency(P, _vals(P, Hl, SCHUR, 0), k=4)
    assert out["cand_bearing"][0] == edge
    ref.check_rows(out, "host outlier world")


def _raw(P, vals, gate_bearing, gate_odom, k, fill=7):
    """The C call with sentinel-filled outputs: (rc, outputs)."""
    cs = P.c_struct()
    opt = bos.options(SCHUR)
    out = bos._edge_check_arrays(P, 8, True, True)
    for a in out.values():
        a.fill(fill)
    rc = bos.lib().bos_plan_mf_edge_consistency(ctypes.byref(cs), ctypes.byref(opt), vals.ctypes.data_as(ctypes.POINTER(ctypes.c_double)),
                                                gate_bearing, gate_odom, k, *bos._edge_check_pointers(out))
    return rc, out


def test_invalid_arguments_touch_nothing():
    P, Hl, _ = _case("mini")
    vals = _vals(P, Hl, SCHUR, 0)
    for gb, go, k in ((np.nan, 0.0, 4), (0.0, np.nan, 4), (-1.0, 0.0, 4), (0.0, -1e-300, 4), (np.inf, 0.0, 4), (0.0, np.inf, 4),
                      (0.0, 0.0, 0), (0.0, 0.0, 9), (0.0, 0.0, -1)):
        rc, out = _raw(P, vals, gb, go, k)
        assert rc == ERR_INVALID, (gb, go, k)
        assert all(np.all(a == 7) for a in out.values()), (gb, go, k)
    rc, out = _raw(P, vals, 0.0, 0.0, 8)
    assert rc == bos.BOS_OK and not any(np.any(out[key] == 7) for key in LIST_KEYS)
    ix, val, count = expected_list(out["bearing_w2"], 0.0, 8)
    assert np.array_equal(out["cand_bearing"], ix) and out["n_over_bearing"][0] == count


def test_fixed_pose_alone():
    """plan.n == 0: no landmark, every odometry edge a self-loop on the fixed pose. P is zero everywhere: padding,
    counts 0, w2 and redundancy NaN, chi2 = z^T Omega z (e = -z)."""
    z = np.array([[0.1, -0.2, 0.05], [0.0, 0.3, -0.1]])
    om = np.tile(np.diag([500.0, 500.0, 5000.0]), (2, 1, 1))
    P = bos.Problem(np.array([[1.0, 2.0, 0.5]]), np.zeros((0, 2)), np.zeros(0, np.int32), np.zeros(0, np.int32), np.zeros(0),
                    np.zeros(2, np.int32), np.zeros(2, np.int32), z, om, 0)
    out = bos.plan_mf_edge_consistency(P, np.zeros(1), k=3)
    assert np.all(out["cand_odom"] == -1) and np.all(out["cand_bearing"] == -1) and out["n_over_odom"] == out["n_over_bearing"] == 0
    assert np.all(np.isneginf(out["cand_odom_w2"])) and np.all(out["cand_odom_rescov"] == 0.0)
    assert np.all(np.isnan(out["odom_w2"])) and np.all(np.isnan(out["odom_redundancy"]))
    assert np.allclose(out["odom_chi2"], np.einsum("mi,mij,mj->m", z, om, z), rtol=1e-14, atol=0.0)
    assert len(out["bearing_w2"]) == 0


def test_null_outputs():
    """Every output may be NULL: the others are what the full call returns."""
    P, Hl, _ = _case("mini")
    vals = _vals(P, Hl, SCHUR, 0)
    full = bos.plan_mf_edge_consistency(P, vals, k=4)
    out = bos.plan_mf_edge_consistency(P, vals, k=4, rows=False)
    assert all(out[r] is None for r in ROW_KEYS)
    assert all(np.array_equal(out[key], full[key]) for key in LIST_KEYS)
