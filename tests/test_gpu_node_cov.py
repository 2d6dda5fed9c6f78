"""Solver.node_covariances() (bos_node_covariances: J+H build, multifrontal factorization, selected inverse,
then per query node the root-path solve, the scatter, the backward sweep over every front and the gather +
projection kernel) against a dense inverse of the system the same call linearised (export_system() right
after it), against the host twin, against pair_covariances() and marginals() on the same handle, and for
non-interference with the GN steps around it. Query nodes, conversion to the pair layout and exact rules:
tests/node_cov_ref.py; reference, error measures and bounds: tests/pair_cov_ref.py."""
import numpy as np
import pytest

import bos
from conftest import C1, MINI
from helpers import gpu_lower
from marginals_ref import TOL_CAP, DenseInverses, sparse_tol
from node_cov_ref import NODE_KEYS, check_column_rules, query_nodes, to_pairs
from pair_cov_ref import PairReference, check_reference, check_refined, dims, pair_jacobian
from test_edge_cov_host import edge_case_world
from test_gpu_pair_cov import PLAN_KW

pytestmark = pytest.mark.gpu

SCHUR, SUPERNODAL = bos.BOS_SOLVER_SCHUR, bos.BOS_SOLVER_SUPERNODAL
ALL_KEYS = NODE_KEYS + ("pose_cov", "landmark_cov")


@pytest.fixture(scope="module")
def c1():
    return bos.load_g2o(C1)


@pytest.fixture(scope="module")
def c1_nodes(c1):
    return query_nodes(c1, SCHUR)[0]


_dense = {}


def _dense_of(P, Hl, vals):
    """The dense inverses of one exported system, shared by the handles that export the same bits."""
    key = (P.N, vals.tobytes())
    if key not in _dense:
        _dense[key] = DenseInverses(P, Hl)
    return _dense[key]


def _same(x, y, keys=ALL_KEYS):
    return all(np.array_equal(x[k], y[k]) for k in keys) and x["solver_info"] == y["solver_info"] == 0


def _accuracy(P, S, what, solver=SCHUR, leaf=0):
    nodes, kinds = query_nodes(P, solver, leaf)
    out = S.node_covariances(nodes, marginals=True)
    rows, cols, vals, _ = S.export_system()
    pose, lm = S.get_state()
    Hl = gpu_lower(rows, cols, vals, P.N)
    a, b, pairs = to_pairs(P, nodes, out)
    ref = PairReference(P, Hl, a, b, pose, lm, dense=_dense_of(P, Hl, vals))
    assert out["solver_info"] == 0
    label = f"node column gpu {what} queries {','.join(kinds)}"
    check_reference(ref, pairs, label)
    check_refined(ref, pairs, label)      # within 8 x the fp64 references' own error of Sigma*
    check_column_rules(P, nodes, out)
    return kinds


@pytest.mark.parametrize("plan", ["schur", "supernodal", "schur_leaf40"])
def test_accuracy_fp64(c1, plan):
    """C1's three plans: the wave class, the block class (fronts of 65-354 rows, k up to 225: several
    pivot blocks) and, in the Schur plan, the folded landmarks' launch."""
    kw = PLAN_KW[plan]
    fronts = bos.plan_mf_fronts(c1, **kw)
    assert (fronts[:, 0] + fronts[:, 1]).max() > 64
    S = bos.Solver(c1, **kw)
    kinds = _accuracy(c1, S, plan, kw["solver"], kw.get("schur_leaf", 0))
    S.close()
    if plan == "schur":
        assert fronts[:, 6].any() and "folded_landmark" in kinds


def test_register_class_alone():
    """bos.synthetic(60, 120, 6): every front has at most 64 rows, so the sweep runs in the wave class only."""
    P = bos.synthetic(60, 120, 6)
    fronts = bos.plan_mf_fronts(P, solver=SCHUR)
    assert (fronts[:, 0] + fronts[:, 1]).max() <= 64
    S = bos.Solver(P, solver=SCHUR)
    _accuracy(P, S, "synthetic 60/120/6", SCHUR)
    S.close()


@pytest.mark.parametrize("solver", [SCHUR, SUPERNODAL])
def test_mini_dataset(solver):
    """n = 18: at most 2 levels."""
    P = bos.load_g2o(MINI)
    S = bos.Solver(P, solver=solver)
    _accuracy(P, S, f"mini solver {solver}", solver)
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


def _pair_scales(P, a, b, pose_cov, lm_cov):
    """(cross, projected) scales [n, 9] of the pairs from the marginal standard deviations, as
    test_gpu_pair_cov.test_gpu_matches_host forms them: sd_i sd_j, and s_u s_v with s = sum |J| sd at P's state."""
    sd = np.concatenate([np.sqrt(np.diagonal(pose_cov, axis1=1, axis2=2)).ravel(), np.sqrt(np.diagonal(lm_cov, axis1=1, axis2=2)).ravel()])
    da, db = dims(P, a, b)
    sc = np.zeros((len(a), 9))
    sp = np.zeros((len(a), 9))
    for q in range(len(a)):
        ia = np.arange(3 * a[q], 3 * a[q] + 3) if a[q] < P.NP else 3 * P.NP + 2 * (a[q] - P.NP) + np.arange(2)
        ib = np.arange(3 * b[q], 3 * b[q] + 3) if b[q] < P.NP else 3 * P.NP + 2 * (b[q] - P.NP) + np.arange(2)
        sc[q, :da[q] * db[q]] = np.outer(sd[ia], sd[ib]).ravel()
        J = pair_jacobian(P, P.pose_xyt, P.lm_xy, a[q], b[q])
        s = (np.abs(J) * np.concatenate([sd[ia], sd[ib]])).sum(axis=1)
        sp[q, :len(s) ** 2] = np.outer(s, s).ravel()
    return sc, sp


def _scaled(x, y, scale):
    d = np.abs(x - y)
    assert np.all(d[scale == 0] == 0.0)
    return float((d[scale > 0] / scale[scale > 0]).max())


@pytest.mark.parametrize("which", ["c1", "c2"])
def test_gpu_matches_host(c1, which):
    """The host twin on the GPU's own exported values gives the GPU's columns within min(sparse tol, 1e-6)
    (projected entries 2 x), the errors scaled by the host's own diagonal blocks. Config 2 (synthetic
    1000 / 2000 / 20) has fronts of 65-128 rows."""
    P = c1 if which == "c1" else bos.synthetic(1000, 2000, 20)
    if which == "c2":
        fronts = bos.plan_mf_fronts(P, solver=SCHUR)
        assert 64 < (fronts[:, 0] + fronts[:, 1]).max() <= 128
    nodes, _ = query_nodes(P, SCHUR)
    if which == "c2":
        nodes = nodes[1:4]
    S = bos.Solver(P)
    out = S.node_covariances(nodes, marginals=True)
    rows, cols, vals, _ = S.export_system()
    S.close()
    assert out["solver_info"] == 0
    host = bos.plan_mf_node_covariances(P, vals, nodes, solver=SCHUR)
    tol, kappa = sparse_tol(P, gpu_lower(rows, cols, vals, P.N))
    bound = min(tol, TOL_CAP)
    a, b, pg = to_pairs(P, nodes, out)
    _, _, ph = to_pairs(P, nodes, host)
    sc, sp = _pair_scales(P, a, b, host["pose_cov"], host["landmark_cov"])
    ec, ep = _scaled(pg["cross"], ph["cross"], sc), _scaled(pg["projected"], ph["projected"], sp)
    eb = 0.0
    for k in ("pose_cov", "landmark_cov"):
        sd = np.sqrt(np.diagonal(host[k], axis1=1, axis2=2))
        eb = max(eb, _scaled(out[k], host[k], sd[:, :, None] * sd[:, None, :]))
    print(f"node column gpu vs host {which}: kappa_1 {kappa:.3g} tol {tol:.3g} blocks {eb:.3g} cross {ec:.3g} projected {ep:.3g}")
    check_column_rules(P, nodes, out)
    assert eb <= bound and ec <= bound and ep <= 2 * bound


def test_agrees_with_pair_covariances(c1, c1_nodes):
    """The same column through pair_covariances() on the same handle: cross within tol, projected within 2 tol."""
    P = c1
    S = bos.Solver(P)
    out = S.node_covariances(c1_nodes, marginals=True)
    a, b, pairs = to_pairs(P, c1_nodes, out)
    pair = S.pair_covariances(a, b)
    rows, cols, vals, _ = S.export_system()
    S.close()
    assert out["solver_info"] == pair["solver_info"] == 0
    tol, _ = sparse_tol(P, gpu_lower(rows, cols, vals, P.N))
    assert tol <= TOL_CAP
    sc, sp = _pair_scales(P, a, b, out["pose_cov"], out["landmark_cov"])
    ec, ep = _scaled(pairs["cross"], pair["cross"], sc), _scaled(pairs["projected"], pair["projected"], sp)
    print(f"node column gpu vs pair route: tol {tol:.3g} cross {ec:.3g} projected {ep:.3g}")
    assert ec <= tol and ep <= 2 * tol


def test_marginals_bit_for_bit(c1, c1_nodes):
    S = bos.Solver(c1)
    out = S.node_covariances(c1_nodes, marginals=True)
    only = S.node_covariances(c1_nodes[:1], cross=False, projected=False, marginals=True)
    pose_cov, lm_cov, info = S.marginals()
    S.close()
    assert out["solver_info"] == info == 0
    assert np.array_equal(out["pose_cov"], pose_cov) and np.array_equal(out["landmark_cov"], lm_cov)
    assert np.array_equal(only["pose_cov"], pose_cov) and np.array_equal(only["landmark_cov"], lm_cov)


def test_deterministic(c1, c1_nodes):
    S = bos.Solver(c1)
    x = S.node_covariances(c1_nodes, marginals=True)
    y = S.node_covariances(c1_nodes, marginals=True)
    S.close()
    assert _same(x, y)


def test_independent_of_company(c1, c1_nodes):
    """A node alone returns the bits it has inside a 6-node call."""
    nodes = c1_nodes[:6]
    assert len(nodes) == 6
    S = bos.Solver(c1)
    full = S.node_covariances(nodes)
    for i in (1, 4, 5):
        alone = S.node_covariances(nodes[i:i + 1])
        assert alone["solver_info"] == 0
        assert all(np.array_equal(alone[k][0], full[k][i]) for k in NODE_KEYS), i
    S.close()


def test_null_outputs(c1, c1_nodes):
    """Every combination of the three output groups returns the same bits for what it returns."""
    S = bos.Solver(c1)
    full = S.node_covariances(c1_nodes, marginals=True)
    groups = {"cross": NODE_KEYS[:2], "projected": NODE_KEYS[2:], "marginals": ("pose_cov", "landmark_cov")}
    for mask in range(8):
        kw = {g: bool(mask >> i & 1) for i, g in enumerate(groups)}
        out = S.node_covariances(c1_nodes, **kw)
        assert out["solver_info"] == 0
        for g, keys in groups.items():
            for k in keys:
                assert (np.array_equal(out[k], full[k]) if kw[g] else out[k] is None), (kw, k)
    S.close()


def test_empty_call_and_bad_ids(c1):
    S = bos.Solver(c1)
    S.step()
    dx = S.last_dx()
    out = S.node_covariances([])
    assert out["cross_pose"].shape == (0, c1.NP, 9) and out["projected_landmark"].shape == (0, c1.NL, 4) and out["solver_info"] == 0
    assert np.array_equal(S.last_dx(), dx)                       # n_nodes = 0 touched nothing
    NP, NL = c1.NP, c1.NL
    for nodes in ([-1], [NP + NL], [0, -1], [NP, NP + NL]):
        with pytest.raises(bos.BosError, match=r"\(-1\)"):
            S.node_covariances(nodes)
    assert np.array_equal(S.last_dx(), dx)
    S.node_covariances([NP])
    with pytest.raises(bos.BosError, match=r"\(-1\)"):
        S.last_dx()                                              # as after bos_marginals
    S.close()


def test_timing(c1, c1_nodes):
    """The phases that ran report > 0; a cross-only call does not run the selected inverse."""
    S = bos.Solver(c1)
    assert S.node_covariances_timing()["node_bytes"] == 0       # nothing allocated before the first call
    S.node_covariances(c1_nodes[1:3], projected=False)
    t = S.node_covariances_timing()
    assert t["node_bytes"] > 0 and t["selinv_ms"] == 0.0
    assert all(t[k] > 0 for k in ("prepare_ms", "jh_ms", "factor_ms", "column_ms", "gather_ms", "download_ms"))
    S.node_covariances(c1_nodes[1:3])
    t = S.node_covariances_timing()
    assert all(t[k] > 0 for k in ("jh_ms", "factor_ms", "selinv_ms", "column_ms", "gather_ms", "download_ms"))
    S.close()


@pytest.mark.parametrize("precision", [bos.BOS_FP64, bos.BOS_FP32])
def test_steps_do_not_see_the_call(c1, c1_nodes, precision):
    """The state is bit-identical across node_covariances(); step, node_covariances, step ends where
    step, step does."""
    A = bos.Solver(c1, precision=precision)
    B = bos.Solver(c1, precision=precision)
    A.step()
    B.step()
    before = A.get_state()
    A.node_covariances(c1_nodes, marginals=True)
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
    with pytest.raises(bos.BosError, match=r"\(-5\).*bos_node_covariances"):
        S.node_covariances([0])
    S.close()
