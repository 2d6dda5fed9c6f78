"""Reference, pair sets and error measures shared by the pair-covariance tests (host and GPU), built on
marginals_ref.DenseInverses and edge_cov_ref's restatement of the two Jacobians.

Outputs (bos.h bos_pair_covariances): [n, 9] arrays, pair q's block row-major in the first rows * cols
entries of row q, the rest exactly 0. Reference values are read out of a dense inverse of the very H the
call linearised, padded with zeros for the fixed pose.

Measures, those of edge_cov_ref.py:
  cross / cov_a / cov_b entry (i, j): |out - ref| / (sd_i sd_j) <= tol = n eps kappa_1(H_s), tol <= 1e-6
  asserted first;
  projected entry (u, v): |out - ref| / (s_u s_v) <= 2 tol, s_u = sum_i |J_ui| sd_i over the joint dofs; J is
  the odometry Jacobian (pose-pose), the bearing Jacobian (pose-landmark) or [I, -I] (landmark-landmark).
Where a scale is zero (only the fixed pose's dofs are involved) the output must be exactly zero.
The refined criterion: the same measures against Sigma* (np.longdouble, J in longdouble), each group
(blocks, cross, projected) within MARGIN = 8 x e_ref, e_ref the larger error of the LU and the Cholesky
fp64 inverses over the same entries."""
import numpy as np

import bos
from edge_cov_ref import bearing_jacobians, odometry_jacobians
from marginals_ref import MARGIN, TOL_CAP, DenseInverses, Reference, ratio

KEYS = ("cross", "projected", "cov_a", "cov_b")
GROUPS = {"blocks": ("cov_a", "cov_b"), "cross": ("cross",), "projected": ("projected",)}


def node_dofs(P, u):
    """Reference dof numbering of node u (pose stix u: u; landmark stix l: NP + l)."""
    u = int(u)
    return list(range(3 * u, 3 * u + 3)) if u < P.NP else list(range(3 * P.NP + 2 * (u - P.NP), 3 * P.NP + 2 * (u - P.NP) + 2))


def dims(P, a, b):
    return np.where(np.asarray(a) < P.NP, 3, 2), np.where(np.asarray(b) < P.NP, 3, 2)


def _pad(x):
    out = np.zeros(9, dtype=x.dtype)
    out[:x.size] = x.ravel()
    return out


def pair_jacobian(P, pose, lm, a, b):
    """J of the projection of pair (a, b) over [dofs of a | dofs of b], in the dtype of pose / lm: the
    odometry prediction a -> b (3 x 6), the bearing of landmark b from pose a (1 x 5), or l_a - l_b (2 x 4)."""
    if a < P.NP and b < P.NP:
        return odometry_jacobians(pose[a][None], pose[b][None])[0]
    if a < P.NP:
        return bearing_jacobians(pose[a][None], lm[b - P.NP][None])
    return np.concatenate([np.eye(2, dtype=pose.dtype), -np.eye(2, dtype=pose.dtype)], axis=1)


def pair_entries(P, full, pose, lm, node_a, node_b):
    """(values, scales): dicts of [n, 9] over KEYS read out of the padded N x N matrix `full`, the
    projection's J evaluated in full's dtype at the state (pose, lm); scale 0 marks both the padding and
    the entries that only the fixed pose's dofs reach."""
    dt = full.dtype
    sd = np.sqrt(np.diag(full))
    pose, lm = pose.astype(dt), lm.astype(dt)
    n = len(node_a)
    val = {k: np.zeros((n, 9), dtype=dt) for k in KEYS}
    scale = {k: np.zeros((n, 9), dtype=dt) for k in KEYS}
    for q, (a, b) in enumerate(zip(node_a, node_b)):
        ia, ib = node_dofs(P, a), node_dofs(P, b)
        iab = ia + ib
        val["cross"][q] = _pad(full[np.ix_(ia, ib)])
        val["cov_a"][q] = _pad(full[np.ix_(ia, ia)])
        val["cov_b"][q] = _pad(full[np.ix_(ib, ib)])
        scale["cross"][q] = _pad(np.outer(sd[ia], sd[ib]))
        scale["cov_a"][q] = _pad(np.outer(sd[ia], sd[ia]))
        scale["cov_b"][q] = _pad(np.outer(sd[ib], sd[ib]))
        J = pair_jacobian(P, pose, lm, a, b)
        s = (np.abs(J) * sd[iab]).sum(axis=1)
        val["projected"][q] = _pad(J @ full[np.ix_(iab, iab)] @ J.T)
        scale["projected"][q] = _pad(np.outer(s, s))
    return val, scale


def scaled_errors(out, val, scale, keys):
    """[n]: per pair the largest scaled error over the entries of `keys`; asserts the exact zeros."""
    err = np.zeros(len(out[keys[0]]))
    for k in keys:
        zero = scale[k] == 0.0
        assert np.all(out[k][zero] == 0.0), f"{k}: an entry outside the block, or of the fixed pose alone, is not exactly zero"
        e = np.zeros(out[k].shape)
        e[~zero] = (np.abs(out[k] - val[k])[~zero] / scale[k][~zero]).astype(np.float64)
        err = np.maximum(err, e.max(axis=1)) if len(e) else err
    return err


class PairReference:
    """Reference values of the pairs (node_a, node_b) of problem P for the lower triangle Hl of its H
    (reference dof numbering) at the state (pose, lm): Sigma_ref = the LU inverse with tol and kappa_1
    (marginals_ref.Reference), and the refined criterion's Sigma* with e_ref per group. `dense`: a
    DenseInverses of the same P and Hl, computed once and shared."""

    def __init__(self, P, Hl, node_a, node_b, pose=None, lm=None, dense=None):
        d = DenseInverses(P, Hl) if dense is None else dense
        base = Reference(P, Hl, dense=d)
        self.tol, self.kappa, self.n = base.tol, base.kappa, base.n
        pose = P.pose_xyt if pose is None else pose
        lm = P.lm_xy if lm is None else lm
        self.val, self.scale = pair_entries(P, d.full(d.lu), pose, lm, node_a, node_b)
        self.star, self.star_scale = pair_entries(P, d.full(d.star), pose, lm, node_a, node_b)
        self.e_lu, self.e_chol = {}, {}
        for X, e in ((d.lu, self.e_lu), (d.chol, self.e_chol)):
            ent = pair_entries(P, d.full(X), pose, lm, node_a, node_b)[0]
            for g, keys in GROUPS.items():
                errs = scaled_errors(ent, self.star, self.star_scale, keys)
                e[g] = float(errs.max()) if len(errs) else 0.0
        self.e_ref = {g: max(self.e_lu[g], self.e_chol[g]) for g in GROUPS}

    def errors(self, out):
        return {g: float(scaled_errors(out, self.val, self.scale, keys).max()) for g, keys in GROUPS.items()}

    def refined_errors(self, out):
        return {g: float(scaled_errors(out, self.star, self.star_scale, keys).max()) for g, keys in GROUPS.items()}


def check_reference(ref, out, label=""):
    """tol <= 1e-6 first; diagonal and cross blocks within tol, projected entries within 2 tol."""
    assert ref.tol <= TOL_CAP
    e = ref.errors(out)
    print(f"  pair covariances {label}: n {ref.n} kappa_1 {ref.kappa:.3g} tol {ref.tol:.3g}: blocks {e['blocks']:.3g} "
          f"cross {e['cross']:.3g} projected {e['projected']:.3g}")
    assert e["blocks"] <= ref.tol
    assert e["cross"] <= ref.tol
    assert e["projected"] <= 2 * ref.tol
    return e


def check_refined(ref, out, label=""):
    """e <= MARGIN e_ref against Sigma* for each group; prints every figure before asserting."""
    e = ref.refined_errors(out)
    for g in GROUPS:
        print(f"  refined {label} {g}: e {e[g]:.3g} e_ref {ref.e_ref[g]:.3g} (lu {ref.e_lu[g]:.3g} / chol {ref.e_chol[g]:.3g}) "
              f"ratio {ratio(e[g], ref.e_ref[g]):.3g}")
    for g in GROUPS:
        assert e[g] <= MARGIN * ref.e_ref[g], (label, g, e[g], ref.e_ref[g], ratio(e[g], ref.e_ref[g]))
    return e


def check_rules(P, node_a, node_b, out, ref=None):
    """The exact rules of bos_pair_covariances on one result, and the bounds that need no reference
    values: |Sigma_ab[i][j]| <= sd_i sd_j (1 + tol) from the call's own diagonal blocks, every variance
    > 0, every pose-pose projected block positive semi-definite up to its own error bound (ref given)."""
    a, b = np.asarray(node_a), np.asarray(node_b)
    da, db = dims(P, a, b)
    fx = P.fixed
    cross, proj, ca, cb = (out[k] for k in KEYS)
    n = len(a)
    for q in range(n):
        A, B = ca[q, :da[q] ** 2].reshape(da[q], da[q]), cb[q, :db[q] ** 2].reshape(db[q], db[q])
        C = cross[q, :da[q] * db[q]].reshape(da[q], db[q])
        assert np.all(ca[q, da[q] ** 2:] == 0.0) and np.all(cb[q, db[q] ** 2:] == 0.0) and np.all(cross[q, da[q] * db[q]:] == 0.0)
        assert np.array_equal(A, A.T) and np.array_equal(B, B.T)            # mirrored lower triangles
        if a[q] == fx:
            assert np.all(A == 0.0) and np.all(C == 0.0)
        else:
            assert np.all(np.diag(A) > 0.0)
        if b[q] == fx:
            assert np.all(B == 0.0) and np.all(C == 0.0)
        else:
            assert np.all(np.diag(B) > 0.0)
        if a[q] == b[q]:
            assert np.array_equal(C, A) and np.array_equal(C, B)
        tol = ref.tol if ref is not None else TOL_CAP
        assert np.all(np.abs(C) <= np.sqrt(np.outer(np.diag(A), np.diag(B))) * (1 + tol))
        free_pair = a[q] != b[q] and not (a[q] == fx and b[q] == fx)
        if da[q] == 3 and db[q] == 3:
            M = proj[q].reshape(3, 3)
            assert np.array_equal(M, M.T)
            if free_pair:
                assert np.all(np.diag(M) > 0.0)
                if ref is not None:   # every entry within 2 tol s_u s_v of a PSD matrix: |error|_2 <= 2 tol (sum_u s_u)^2
                    s = np.sqrt(np.diag(ref.scale["projected"][q].reshape(3, 3).astype(np.float64)))
                    assert np.linalg.eigvalsh(M)[0] >= -2 * ref.tol * s.sum() ** 2
        elif da[q] == 3:
            assert np.all(proj[q, 1:] == 0.0)
            if free_pair:
                assert proj[q, 0] > 0.0
        else:
            M = proj[q, :4].reshape(2, 2)
            assert np.all(proj[q, 4:] == 0.0) and np.array_equal(M, M.T)
            if free_pair:
                assert np.all(np.diag(M) > 0.0)
    # duplicates: identical bits; the reversed pair: the exact transpose
    seen = {}
    for q in range(n):
        key = (int(a[q]), int(b[q]))
        f = seen.setdefault(key, q)
        if f != q:
            assert all(np.array_equal(out[k][q], out[k][f]) for k in KEYS), (q, f)
        g = seen.get((key[1], key[0]))
        if g is not None and g != q and key[0] != key[1]:
            Cq = cross[q, :da[q] * db[q]].reshape(da[q], db[q])
            Cg = cross[g, :da[g] * db[g]].reshape(da[g], db[g])
            assert np.array_equal(Cq, Cg.T), (q, g)
            assert np.array_equal(ca[q], cb[g]) and np.array_equal(cb[q], ca[g])


def random_pairs(P, rng, n_each):
    """n_each seeded random pairs of each kind: pose-pose, pose-landmark, landmark-landmark."""
    a = np.concatenate([rng.integers(0, P.NP, n_each), rng.integers(0, P.NP, n_each), P.NP + rng.integers(0, P.NL, n_each)])
    b = np.concatenate([rng.integers(0, P.NP, n_each), P.NP + rng.integers(0, P.NL, n_each), P.NP + rng.integers(0, P.NL, n_each)])
    return a.astype(np.int32), b.astype(np.int32)


CLASSES = ("root_from_two_subtrees", "same_supernode", "ancestor", "folded_landmark_unobserved", "fixed_pose_pose",
           "fixed_pose_landmark", "self_pair", "duplicate", "reverse")


def constructed_pairs(P, solver, schur_leaf=0, seed=5, per_class=4):
    """(node_a, node_b, classes): pairs of each constructed kind found with plan_pair_paths in a seeded
    candidate pool; classes maps each name of CLASSES to the indices (into the returned arrays) of its
    pairs, empty where the plan has none."""
    rng = np.random.default_rng(seed)
    ca, cb = random_pairs(P, rng, 3000)
    paths = bos.plan_pair_paths(P, ca, cb, solver=solver, schur_leaf=schur_leaf)
    fronts = bos.plan_mf_fronts(P, solver=solver, schur_leaf=schur_leaf)
    sa, sb, lca = paths[:, 0], paths[:, 1], paths[:, 2]
    ok = lca >= 0
    root = np.zeros(len(ca), dtype=bool)
    root[ok] = (fronts[lca[ok], 3] < 0) | (fronts[lca[ok], 1] == 0)
    observed = set(zip(P.b_pose.tolist(), (P.b_lm + P.NP).tolist()))
    folded = np.zeros(len(ca), dtype=bool)
    mixed = (ca < P.NP) & (cb >= P.NP) & ok
    folded[mixed] = fronts[sb[mixed], 6] == 1
    folded &= np.array([(int(x), int(y)) not in observed for x, y in zip(ca, cb)])
    cand = {"root_from_two_subtrees": ok & root & (lca != sa) & (lca != sb),
            "same_supernode": ok & (sa == sb) & (ca != cb),
            "ancestor": ok & (sa != sb) & ((lca == sa) | (lca == sb)),
            "folded_landmark_unobserved": folded}
    a, b, classes = [], [], {}

    def add(name, pa, pb):
        classes[name] = list(range(len(a), len(a) + len(pa)))
        a.extend(int(x) for x in pa)
        b.extend(int(x) for x in pb)

    for name, mask in cand.items():
        idx = np.nonzero(mask)[0][:per_class]
        add(name, ca[idx], cb[idx])
    free = [p for p in range(P.NP) if p != P.fixed]
    fx = P.fixed
    add("fixed_pose_pose", [fx, free[0], fx], [free[-1], fx, fx])
    add("fixed_pose_landmark", [fx, fx], [P.NP, P.NP + P.NL - 1])
    add("self_pair", [free[0], P.NP + P.NL // 2], [free[0], P.NP + P.NL // 2])
    add("duplicate", [free[1], free[1], P.NP + 1, P.NP + 1], [free[-2], free[-2], P.NP + P.NL - 2, P.NP + P.NL - 2])
    add("reverse", [free[-2], P.NP + P.NL - 2], [free[1], P.NP + 1])
    return np.array(a, dtype=np.int32), np.array(b, dtype=np.int32), classes


def pair_set(P, solver, schur_leaf=0, n_each=200, seed=3):
    """The tests' seeded pair set: n_each random pairs of each kind, then the constructed ones (their
    class indices shifted accordingly)."""
    ra, rb = random_pairs(P, np.random.default_rng(seed), n_each)
    ka, kb, classes = constructed_pairs(P, solver, schur_leaf)
    classes = {k: [i + len(ra) for i in v] for k, v in classes.items()}
    return np.concatenate([ra, ka]), np.concatenate([rb, kb]), classes
