"""Solver.pair_covariances() (bos_pair_covariances: J+H build, multifrontal factorization, one root-path
solve per distinct node, products over the common tails, projection kernel) against a dense inverse of
the system the same call linearised (export_system() right after it), against the host twin, against
edge_covariances() and marginals() on the same handle, and for non-interference with the GN steps around
it. Reference, pair sets, error measures and bounds: tests/pair_cov_ref.py."""
import numpy as np
import pytest

import bos
from conftest import C1, MINI
from helpers import gpu_lower
from marginals_ref import TOL_CAP, DenseInverses, sparse_tol
from pair_cov_ref import (KEYS, PairReference, check_reference, check_refined, check_rules, dims, node_dofs, pair_jacobian,
                          pair_set, random_pairs)
from test_edge_cov_host import edge_case_world

pytestmark = pytest.mark.gpu

SCHUR, SUPERNODAL = bos.BOS_SOLVER_SCHUR, bos.BOS_SOLVER_SUPERNODAL


@pytest.fixture(scope="module")
def c1():
    return bos.load_g2o(C1)


@pytest.fixture(scope="module")
def c1_pairs(c1):
    """2 000 seeded pairs on C1, a third of each kind."""
    a, b = random_pairs(c1, np.random.default_rng(17), 667)
    return a[:2000], b[:2000]


_dense = {}


def _dense_of(P, Hl, vals):
    """The dense inverses of one exported system, shared by the handles that export the same bits."""
    key = (P.N, vals.tobytes())
    if key not in _dense:
        _dense[key] = DenseInverses(P, Hl)
    return _dense[key]


def _same(x, y, keys=KEYS):
    return all(np.array_equal(x[k], y[k]) for k in keys) and x["solver_info"] == y["solver_info"] == 0


def _accuracy(P, S, what, solver=SCHUR, leaf=0):
    a, b, _ = pair_set(P, solver, leaf)
    out = S.pair_covariances(a, b)
    rows, cols, vals, _ = S.export_system()
    pose, lm = S.get_state()
    Hl = gpu_lower(rows, cols, vals, P.N)
    ref = PairReference(P, Hl, a, b, pose, lm, dense=_dense_of(P, Hl, vals))
    assert out["solver_info"] == 0
    check_reference(ref, out, f"gpu {what}")
    check_refined(ref, out, f"gpu {what}")      # within 8 x the fp64 references' own error of Sigma*
    check_rules(P, a, b, out, ref)
    return out


PLAN_KW = {"schur": dict(solver=SCHUR), "supernodal": dict(solver=SUPERNODAL), "schur_leaf40": dict(solver=SCHUR, schur_leaf=40)}


@pytest.mark.parametrize("plan", ["schur", "supernodal", "schur_leaf40"])
def test_accuracy_fp64(c1, plan):
    """C1's three plans: paths through folded landmarks, wave fronts and the fronts of 65-354 rows (k up
    to 225) that keep w in LDS."""
    kw = PLAN_KW[plan]
    fronts = bos.plan_mf_fronts(c1, **kw)
    assert (fronts[:, 0] + fronts[:, 1]).max() > 64
    S = bos.Solver(c1, **kw)
    _accuracy(c1, S, plan, kw["solver"], kw.get("schur_leaf", 0))
    S.close()


@pytest.mark.parametrize("solver", [SCHUR, SUPERNODAL])
def test_mini_dataset(solver):
    """n = 18: a path of at most 2 fronts."""
    P = bos.load_g2o(MINI)
    S = bos.Solver(P, solver=solver)
    _accuracy(P, S, f"mini solver {solver}", solver)
    S.close()


def test_register_class_alone():
    """bos.synthetic(60, 120, 6): every front has at most 64 rows, so every path runs in the register
    class only; against its own dense reference."""
    P = bos.synthetic(60, 120, 6)
    fronts = bos.plan_mf_fronts(P, solver=SCHUR)
    assert (fronts[:, 0] + fronts[:, 1]).max() <= 64
    S = bos.Solver(P, solver=SCHUR)
    _accuracy(P, S, "synthetic 60/120/6", SCHUR)
    S.close()


@pytest.mark.parametrize("solver", [SCHUR, SUPERNODAL])
def test_edge_case_world(c1, solver):
    P = edge_case_world(c1)
    S = bos.Solver(P, solver=solver)
    _accuracy(P, S, f"edge cases solver {solver}", solver)
    S.close()


def test_accuracy_fp32(c1):
    """fp32 J+H, fp64 factor; J of the projection from the fp64 master state: against its own exported system."""
    S = bos.Solver(c1, precision=bos.BOS_FP32)
    _accuracy(c1, S, "fp32")
    S.close()


def test_accuracy_after_steps(c1):
    """At the estimate of 10 GN iterations, the stream still busy with the last step when asked."""
    S = bos.Solver(c1)
    S.step_n(10)
    _accuracy(c1, S, "after 10 steps")
    S.close()


@pytest.mark.parametrize("which", ["c1", "c2"])
def test_gpu_matches_host(c1, which):
    """The host twin on the GPU's own exported values gives the GPU's results on 2 000 seeded pairs, within
    min(sparse tol, 1e-6) (projected entries 2 x), the errors scaled by the host's own diagonal blocks.
    Config 2 (synthetic 1000 / 2000 / 20) has fronts of 65-96 rows."""
    P = c1 if which == "c1" else bos.synthetic(1000, 2000, 20)
    if which == "c2":
        fronts = bos.plan_mf_fronts(P, solver=SCHUR)
        assert 64 < (fronts[:, 0] + fronts[:, 1]).max() <= 128
    a, b = random_pairs(P, np.random.default_rng(23), 667)
    a, b = a[:2000], b[:2000]
    S = bos.Solver(P)
    out = S.pair_covariances(a, b)
    rows, cols, vals, _ = S.export_system()
    S.close()
    assert out["solver_info"] == 0
    host = bos.plan_mf_pair_covariances(P, vals, a, b, solver=SCHUR)
    tol, kappa = sparse_tol(P, gpu_lower(rows, cols, vals, P.N))
    bound = min(tol, TOL_CAP)
    da, db = dims(P, a, b)
    e = {k: 0.0 for k in KEYS}
    for q in range(len(a)):
        sa = np.sqrt(np.diag(host["cov_a"][q, :da[q] ** 2].reshape(da[q], da[q])))
        sb = np.sqrt(np.diag(host["cov_b"][q, :db[q] ** 2].reshape(db[q], db[q])))
        scales = {"cross": np.outer(sa, sb), "cov_a": np.outer(sa, sa), "cov_b": np.outer(sb, sb)}
        for k, sc in scales.items():
            d = np.abs(out[k][q, :sc.size] - host[k][q, :sc.size]).reshape(sc.shape)
            assert np.all(d[sc == 0] == 0.0)
            if (sc > 0).any():
                e[k] = max(e[k], float((d[sc > 0] / sc[sc > 0]).max()))
        # projected: s_u s_v with J at P's state and the host's standard deviations, as pair_cov_ref does
        J = pair_jacobian(P, P.pose_xyt, P.lm_xy, a[q], b[q])
        s = (np.abs(J) * np.concatenate([sa, sb])).sum(axis=1)
        sc = np.zeros(9)
        sc[:len(s) ** 2] = np.outer(s, s).ravel()
        d = np.abs(out["projected"][q] - host["projected"][q])
        assert np.all(d[sc == 0] == 0.0)
        if (sc > 0).any():
            e["projected"] = max(e["projected"], float((d[sc > 0] / sc[sc > 0]).max()))
    print(f"pair covariances gpu vs host {which}: kappa_1 {kappa:.3g} tol {tol:.3g} " + " ".join(f"{k} {v:.3g}" for k, v in e.items()))
    check_rules(P, a, b, out)
    assert e["cross"] <= bound and e["cov_a"] <= bound and e["cov_b"] <= bound and e["projected"] <= 2 * bound


def test_edges_as_queries(c1):
    """The problem's own edges as queries agree with edge_covariances() on the same handle within tol
    (cross) and 2 tol (projected); cov_a / cov_b agree with marginals() within tol."""
    P = c1
    a = np.concatenate([P.b_pose, P.o_src]).astype(np.int32)
    b = np.concatenate([P.b_lm + P.NP, P.o_dst]).astype(np.int32)
    S = bos.Solver(P)
    out = S.pair_covariances(a, b)
    edge = S.edge_covariances()
    pose_cov, lm_cov, info = S.marginals()
    rows, cols, vals, _ = S.export_system()
    S.close()
    assert out["solver_info"] == edge["solver_info"] == info == 0
    tol, _ = sparse_tol(P, gpu_lower(rows, cols, vals, P.N))
    assert tol <= TOL_CAP
    from edge_cov_ref import bearing_jacobians, odometry_jacobians
    Mb = len(P.b_z)
    sd = np.concatenate([np.sqrt(np.diagonal(pose_cov, axis1=1, axis2=2)).ravel(), np.sqrt(np.diagonal(lm_cov, axis1=1, axis2=2)).ravel()])
    Jb = bearing_jacobians(P.pose_xyt[P.b_pose], P.lm_xy[P.b_lm])
    Jo = odometry_jacobians(P.pose_xyt[P.o_src], P.pose_xyt[P.o_dst])
    ec = ep = eb = 0.0
    for q in range(len(a)):
        ia, ib = node_dofs(P, a[q]), node_dofs(P, b[q])
        sc = np.outer(sd[ia], sd[ib])
        C = out["cross"][q, :sc.size].reshape(sc.shape)
        Ce = edge["bearing_cross"][q] if q < Mb else edge["odom_cross"][q - Mb]
        if q < Mb:
            s = (np.abs(Jb[q]) * sd[ia + ib]).sum()
            pe, ps = np.atleast_1d(abs(out["projected"][q, 0] - edge["bearing_var"][q])), np.atleast_1d(s * s)
        else:
            s = (np.abs(Jo[q - Mb]) * sd[ia + ib]).sum(axis=1)
            pe, ps = np.abs(out["projected"][q].reshape(3, 3) - edge["odom_cov"][q - Mb]), np.outer(s, s)
        assert np.all(C[sc == 0] == 0.0) and np.all(pe[ps == 0] == 0.0)
        if (sc > 0).any():
            ec = max(ec, float((np.abs(C - Ce)[sc > 0] / sc[sc > 0]).max()))
        ep = max(ep, float((pe[ps > 0] / ps[ps > 0]).max()))
        for key, u, idx in (("cov_a", a[q], ia), ("cov_b", b[q], ib)):
            M = pose_cov[u] if u < P.NP else lm_cov[u - P.NP]
            A = out[key][q, :len(idx) ** 2].reshape(len(idx), len(idx))
            if u == P.fixed:
                assert np.all(A == 0.0)
            else:
                eb = max(eb, float((np.abs(A - M) / np.outer(sd[idx], sd[idx])).max()))
    print(f"pair covariances gpu, edges as queries: tol {tol:.3g} blocks {eb:.3g} cross {ec:.3g} projected {ep:.3g}")
    assert eb <= tol and ec <= tol and ep <= 2 * tol


def test_deterministic(c1, c1_pairs):
    S = bos.Solver(c1)
    x = S.pair_covariances(*c1_pairs)
    y = S.pair_covariances(*c1_pairs)
    S.close()
    assert _same(x, y)


def test_independent_of_company(c1, c1_pairs):
    """A query's bits are the same alone, inside the 2 000-pair call, and when that call runs in batches
    of at most 7 distinct nodes."""
    a, b = c1_pairs
    S = bos.Solver(c1)
    full = S.pair_covariances(a, b)
    S.debug_set_pair_batch(7)
    split = S.pair_covariances(a, b)
    S.debug_set_pair_batch(0)
    assert _same(full, split)
    for q in (0, 700, 1400, 1999):
        alone = S.pair_covariances(a[q:q + 1], b[q:q + 1])
        assert alone["solver_info"] == 0
        assert all(np.array_equal(alone[k][0], full[k][q]) for k in KEYS), q
    S.close()


def test_null_outputs(c1, c1_pairs):
    """Every combination of the three output groups returns the same bits for what it returns."""
    a, b = c1_pairs[0][:300], c1_pairs[1][:300]
    S = bos.Solver(c1)
    full = S.pair_covariances(a, b)
    groups = {"cross": ("cross",), "projected": ("projected",), "blocks": ("cov_a", "cov_b")}
    for mask in range(8):
        kw = {g: bool(mask >> i & 1) for i, g in enumerate(groups)}
        out = S.pair_covariances(a, b, **kw)
        assert out["solver_info"] == 0
        for g, keys in groups.items():
            for k in keys:
                assert (np.array_equal(out[k], full[k]) if kw[g] else out[k] is None), (kw, k)
    S.close()


def test_empty_call_and_bad_ids(c1):
    S = bos.Solver(c1)
    S.step()
    dx = S.last_dx()
    out = S.pair_covariances([], [])
    assert all(out[k].shape == (0, 9) for k in KEYS) and out["solver_info"] == 0
    assert np.array_equal(S.last_dx(), dx)                       # n_pairs = 0 touched nothing
    NP, NL = c1.NP, c1.NL
    for a, b in (([-1], [0]), ([0], [NP + NL]), ([NP + NL], [NP]), ([NP], [0]), ([0, NP + 1], [1, 2])):
        with pytest.raises(bos.BosError, match=r"\(-1\)"):
            S.pair_covariances(a, b)
    assert np.array_equal(S.last_dx(), dx)
    S.pair_covariances([0], [NP])
    with pytest.raises(bos.BosError, match=r"\(-1\)"):
        S.last_dx()                                              # as after bos_marginals
    t = S.pair_covariances_timing()
    assert t["pair_bytes"] > 0 and t["factor_ms"] > 0 and t["path_ms"] > 0
    S.close()


@pytest.mark.parametrize("precision", [bos.BOS_FP64, bos.BOS_FP32])
def test_steps_do_not_see_the_call(c1, c1_pairs, precision):
    """The state is bit-identical across pair_covariances(); step, pair_covariances, step ends where
    step, step does."""
    A = bos.Solver(c1, precision=precision)
    B = bos.Solver(c1, precision=precision)
    A.step()
    B.step()
    before = A.get_state()
    A.pair_covariances(*c1_pairs)
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


@pytest.mark.parametrize("kind", ["dense", "rf", "communicator"])
def test_unsupported_handles(c1, kind):
    kw = {"dense": dict(solver=bos.BOS_SOLVER_DENSE_CHOL), "rf": dict(solver=bos.BOS_SOLVER_ROCSOLVER_RF),
          "communicator": dict(solver=SCHUR, rank=0, world_size=1, nccl_id=bos.nccl_unique_id())}[kind]
    S = bos.Solver(c1, **kw)
    with pytest.raises(bos.BosError, match=r"\(-5\).*bos_pair_covariances"):
        S.pair_covariances([0], [1])
    S.close()
