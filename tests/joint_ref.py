"""Reference, hypotheses and checks shared by the joint-compatibility tests (host and GPU).

Quantities (bos.h bos_joint_compatibility), for a hypothesis of m pairings (pose p_i, landmark l_i, z_i, omega_i)
with N_i the five reference dofs [p_i | l_i]:
  e_ref   = associate_ref's: arctan2 of the landmark in the pose's frame, minus z, wrapped
  J_i     = edge_cov_ref.bearing_jacobians (1 x 5)
  S_ref   entry (i, j) = J_i Sigma_ref[N_i, N_j] J_j^T + delta_ij / omega_i, Sigma_ref the dense LU inverse of the H
            the call linearised (marginals_ref.DenseInverses), zero-padded for the fixed pose
  nis_ref = e_ref^T S*^-1 e_ref on every leading block, S* as S_ref from Sigma*, all in np.longdouble
Bounds:
  |S_ij - S_ref,ij| <= 2 tol s_i s_j, s_i = sum |J_i| sd over N_i, tol = n eps kappa_1 (tol <= TOL_CAP asserted
  first), and the refined criterion: the same measure against S* within MARGIN x e_ref, e_ref the larger error
  of the LU and the Cholesky fp64 inverses over the same entries;
  |nis - nis_ref| <= 2 tol (sum_i |x_i| s_i)^2 + 64 eps m kappa_2(S_ref) nis_ref, x = S_ref^-1 e_ref, per leading
  block: the first-order perturbation of e^T S^-1 e under the entry bounds, plus the backward error of the
  Cholesky solve. For m = 1 it is associate_ref's bound.
Conditions on the inputs, asserted before anything is compared: every |e_ref| <= 1 rad (no wrap exclusions),
every kappa_2(S_ref) <= KAPPA2_CAP.

ldl_prefix and s_offdiag restate the call's recurrence and its S-entry order with NumPy float64 scalars (IEEE,
no contraction): they reproduce the call's bits."""
import numpy as np

import bos
from associate_ref import observed_landmark, predicted_bearings, wrap
from edge_cov_ref import bearing_jacobians
from helpers import EPS
from marginals_ref import MARGIN, TOL_CAP, DenseInverses, Reference, ratio
from pair_cov_ref import constructed_pairs, node_dofs

KAPPA2_CAP = 1e6
E_CAP = 1.0
OMEGAS = (1.0, 25.0, 1e4)


# ---- NumPy restatements --------------------------------------------------------------------------------
def ldl_prefix(S, e):
    """prefix_nis of one hypothesis from its returned S [m, m] and e [m], bit for bit."""
    m = len(e)
    A = np.array(S, dtype=np.float64)
    y = np.array(e, dtype=np.float64)
    out = np.full(m, np.nan)
    prev = np.float64(0.0)
    with np.errstate(all="ignore"):
        for k in range(m):
            D = A[k, k]
            if not (np.isfinite(D) and D > 0.0):
                break
            for i in range(k + 1, m):
                l = A[i, k] / D
                for j in range(k + 1, i + 1):
                    A[i, j] = A[i, j] - l * A[j, k]
                y[i] = y[i] - l * y[k]
            prev = prev + (y[k] * y[k]) / D
            out[k] = prev
    return out


def s_offdiag(C, Ji, Jj):
    """J_i C J_j^T in the call's order: t = C J_j^T, every entry an ascending sum, then J_i t ascending."""
    C, Ji, Jj = np.asarray(C, dtype=np.float64), np.asarray(Ji, dtype=np.float64), np.asarray(Jj, dtype=np.float64)
    t = []
    for r in range(5):
        acc = C[r, 0] * Jj[0]
        for c in range(1, 5):
            acc = acc + C[r, c] * Jj[c]
        t.append(acc)
    s = Ji[0] * t[0]
    for r in range(1, 5):
        s = s + Ji[r] * t[r]
    return s


# ---- hypotheses ----------------------------------------------------------------------------------------
class Hypotheses:
    """The flat arrays of a call, and names for the hypotheses the tests look at."""

    def __init__(self):
        self.start, self.pose, self.landmark, self.z, self.omega, self.index = [0], [], [], [], [], {}

    def add(self, name, pose, landmark, z, omega):
        self.index[name] = len(self.start) - 1
        self.pose += [int(p) for p in pose]
        self.landmark += [int(l) for l in landmark]
        self.z += [float(x) for x in z]
        self.omega += [float(x) for x in omega]
        self.start.append(len(self.pose))

    def arrays(self):
        return (np.array(self.start, dtype=np.int32), np.array(self.pose, dtype=np.int32), np.array(self.landmark, dtype=np.int32),
                np.array(self.z), np.array(self.omega))

    def __len__(self):
        return len(self.start) - 1

    def one(self, h):
        """(pose, landmark, z, omega) of hypothesis h"""
        s, p, l, z, om = self.arrays()
        return p[s[h]:s[h + 1]], l[s[h]:s[h + 1]], z[s[h]:s[h + 1]], om[s[h]:s[h + 1]]

    def subset(self, hs):
        """The flat arrays of the hypotheses hs, in that order."""
        parts = [self.one(h) for h in hs]
        start = np.zeros(len(hs) + 1, dtype=np.int32)
        start[1:] = np.cumsum([len(p[0]) for p in parts])
        cat = lambda i, dt: np.concatenate([p[i] for p in parts]).astype(dt) if parts else np.zeros(0, dtype=dt)
        return start, cat(0, np.int32), cat(1, np.int32), cat(2, np.float64), cat(3, np.float64)


PREFIXES = (1, 2, 3, 31)


def make_hypotheses(P, state, solver, leaf=0, seed=11):
    """The tests' hypotheses at the state (pose_xyt, lm_xy): z = the predicted bearing + 0.01 (1 + i mod 5) (-1)^i
    and omega cycling over OMEGAS, i the pairing's index in its hypothesis. Names (Hypotheses.index): empty, single,
    one_pose_two_landmarks, three_poses, m32_one_pose, m32_random, fixed_pose, shared_landmark, pairing_twice,
    prefix_1 / _2 / _3 / _31 (of m32_one_pose), repeat (of m32_random)."""
    pose_xyt, lm_xy = state
    rng = np.random.default_rng(seed)
    free = [p for p in range(P.NP) if p != P.fixed]
    H = Hypotheses()

    def add(name, poses, lms):
        z = [predicted_bearings(pose_xyt, lm_xy, int(p))[int(l)] + 0.01 * (1 + i % 5) * (-1) ** i for i, (p, l) in enumerate(zip(poses, lms))]
        H.add(name, poses, lms, z, [OMEGAS[i % 3] for i in range(len(poses))])

    a = next(p for p in free if np.any(P.b_pose == p))
    la = observed_landmark(P, a)
    add("empty", [], [])
    add("single", [a], [la])
    add("one_pose_two_landmarks", [a, a], [la, (la + 1) % P.NL])
    # three poses whose paths meet high in the tree: a root_from_two_subtrees pose pair and an ancestor pair's pose
    ca, cb, classes = constructed_pairs(P, solver, leaf)
    three = []
    for name in ("root_from_two_subtrees", "ancestor", "same_supernode"):
        for q in classes[name]:
            three += [int(u) for u in (ca[q], cb[q]) if u < P.NP and u != P.fixed and int(u) not in three]
    three = (three + [p for p in (free[0], free[len(free) // 2], free[-1]) if p not in three])[:3]
    add("three_poses", three, [observed_landmark(P, p) for p in three])
    add("m32_one_pose", [a] * 32, [(la + i) % P.NL for i in range(32)])
    add("m32_random", rng.choice(free, 32), rng.integers(0, P.NL, 32))
    add("fixed_pose", [P.fixed, free[-1]], [observed_landmark(P, P.fixed), observed_landmark(P, free[-1])])
    add("shared_landmark", [a, free[-1]], [la, la])
    add("pairing_twice", [a, free[-1], a], [la, (la + 1) % P.NL, la])
    p32, l32, z32, o32 = H.one(H.index["m32_one_pose"])
    for k in PREFIXES:
        H.add(f"prefix_{k}", p32[:k], l32[:k], z32[:k], o32[:k])
    H.add("repeat", *H.one(H.index["m32_random"]))
    return H


# ---- reference -----------------------------------------------------------------------------------------
def _chol_prefix(S, e):
    """e^T S^-1 e on every leading block of S, in S's dtype (np.longdouble): with S = L L^T and L y = e the
    k-th value is sum over i <= k of y_i^2."""
    m = len(e)
    L = np.zeros_like(S)
    y = np.zeros_like(e)
    for i in range(m):
        for j in range(i + 1):
            v = S[i, j] - (L[i, :j] * L[j, :j]).sum()
            L[i, j] = np.sqrt(v) if i == j else v / L[j, j]
        y[i] = (e[i] - (L[i, :i] * y[:i]).sum()) / L[i, i]
    return np.cumsum(y * y)


class JointReference:
    """S_ref, e_ref, nis_ref and the bounds for the hypotheses (flat arrays start, pose, landmark, z, omega) of
    problem P against the lower triangle Hl of its H at the state (pose_xyt, lm_xy); dense: a shared
    DenseInverses."""

    def __init__(self, P, Hl, start, pose, landmark, z, omega, pose_xyt=None, lm_xy=None, dense=None):
        d = DenseInverses(P, Hl) if dense is None else dense
        base = Reference(P, Hl, dense=d)
        self.tol, self.kappa, self.n = base.tol, base.kappa, base.n
        pose_xyt = P.pose_xyt if pose_xyt is None else pose_xyt
        lm_xy = P.lm_xy if lm_xy is None else lm_xy
        omega = np.ones(len(pose)) if omega is None else np.asarray(omega, dtype=np.float64)
        self.start = np.asarray(start)
        full = {k: d.full(X) for k, X in (("lu", d.lu), ("chol", d.chol), ("star", d.star))}
        sd, sd_star = np.sqrt(np.diag(full["lu"])), np.sqrt(np.diag(full["star"]))
        ld = np.longdouble
        self.S, self.S_star, self.s, self.s_star, self.e, self.nis, self.bound, self.kappa2 = [], [], [], [], [], [], [], []
        self.e_lu = self.e_chol = 0.0
        for h in range(len(self.start) - 1):
            q = slice(self.start[h], self.start[h + 1])
            p, l, m = np.asarray(pose[q]), np.asarray(landmark[q]), self.start[h + 1] - self.start[h]
            if m == 0:
                for lst in (self.S, self.S_star):
                    lst.append(np.zeros((0, 0)))
                for lst in (self.s, self.s_star, self.e, self.nis, self.bound):
                    lst.append(np.zeros(0))
                self.kappa2.append(1.0)
                continue
            dofs = np.array([node_dofs(P, a) + node_dofs(P, P.NP + b) for a, b in zip(p, l)])          # [m, 5]
            flat = dofs.ravel()
            J = bearing_jacobians(pose_xyt[p], lm_xy[l])                                                 # [m, 5]
            Jl = bearing_jacobians(pose_xyt[p].astype(ld), lm_xy[l].astype(ld))
            R = np.diag(1.0 / omega[q])

            def S_of(X, Jx):
                blk = X[np.ix_(flat, flat)].reshape(m, 5, m, 5)
                return np.einsum("ia,iajb,jb->ij", Jx.astype(X.dtype), blk, Jx.astype(X.dtype)) + R.astype(X.dtype)

            S = S_of(full["lu"], J)
            Ss = S_of(full["star"], Jl)
            s = (np.abs(J) * sd[dofs]).sum(axis=1)
            ss = (np.abs(Jl) * sd_star[dofs]).sum(axis=1).astype(np.float64)
            e = np.array([wrap(predicted_bearings(pose_xyt, lm_xy, int(a))[int(b)] - zq) for a, b, zq in zip(p, l, z[q])]).ravel()
            self.e_lu = max(self.e_lu, self._scaled(S, Ss, ss))
            self.e_chol = max(self.e_chol, self._scaled(S_of(full["chol"], J), Ss, ss))
            nis = _chol_prefix(Ss, e.astype(ld)).astype(np.float64)
            bound = np.zeros(m)
            for k in range(m):
                Sk, ek = S[:k + 1, :k + 1], e[:k + 1]
                x = np.linalg.solve(Sk, ek)
                bound[k] = 2 * self.tol * (np.abs(x) * s[:k + 1]).sum() ** 2 + 64 * EPS * (k + 1) * np.linalg.cond(Sk) * nis[k]
            self.S.append(S); self.S_star.append(Ss); self.s.append(s); self.s_star.append(ss); self.e.append(e)
            self.nis.append(nis); self.bound.append(bound); self.kappa2.append(float(np.linalg.cond(S)))
        self.e_ref = max(self.e_lu, self.e_chol)

    @staticmethod
    def _scaled(S, ref, s):
        sc = np.outer(s, s)
        return float((np.abs(S - ref).astype(np.float64) / sc).max()) if sc.size else 0.0

    def check_inputs(self):
        assert self.tol <= TOL_CAP
        worst_e = max([float(np.abs(e).max()) for e in self.e if len(e)] + [0.0])
        print(f"  joint inputs: tol {self.tol:.3g} kappa_1 {self.kappa:.3g} worst |e_ref| {worst_e:.3g} worst kappa_2(S_ref) {max(self.kappa2):.3g}")
        assert worst_e <= E_CAP
        assert max(self.kappa2) <= KAPPA2_CAP

    def check(self, out, label=""):
        """Prints every figure, then asserts the bounds on S, the refined criterion, e and the prefix NIS."""
        self.check_inputs()
        eS = eR = eN = eE = 0.0
        for h in range(len(self.start) - 1):
            q = slice(self.start[h], self.start[h + 1])
            if self.start[h + 1] == self.start[h]:
                assert out["joint_nis"][h] == 0.0 and out["innovation_cov"][h].shape == (0, 0)
                continue
            S = out["innovation_cov"][h]
            assert np.array_equal(S, S.T)
            eS = max(eS, self._scaled(S, self.S[h], self.s[h]))
            eR = max(eR, self._scaled(S, self.S_star[h], self.s_star[h]))
            eE = max(eE, float(np.abs(out["innovation"][q] - self.e[h]).max()))
            d = np.abs(out["prefix_nis"][q] - self.nis[h])
            eN = max(eN, float((d / self.bound[h]).max()))
            assert out["joint_nis"][h] == out["prefix_nis"][q][-1]
        print(f"  joint {label}: S {eS:.3g} of 2 tol {2 * self.tol:.3g}; refined {eR:.3g} e_ref {self.e_ref:.3g} (lu {self.e_lu:.3g} / "
              f"chol {self.e_chol:.3g}) ratio {ratio(eR, self.e_ref):.3g}; e {eE:.3g}; worst |nis - ref| / bound {eN:.3g}")
        assert eS <= 2 * self.tol
        assert eR <= MARGIN * self.e_ref
        assert eE <= 64 * EPS          # |e| <= 1: atan2 and the difference, a few ulp of pi
        assert eN <= 1.0
        return {"S": eS, "refined": eR, "nis": eN}


def check_recurrence(out):
    """prefix_nis from the returned e and S by ldl_prefix, bit for bit; S bit-symmetric; joint_nis the last prefix."""
    start = out["hyp_start"]
    for h in range(len(start) - 1):
        q = slice(start[h], start[h + 1])
        S = out["innovation_cov"][h]
        assert np.array_equal(S, S.T)
        assert np.array_equal(ldl_prefix(S, out["innovation"][q]), out["prefix_nis"][q], equal_nan=True), h
        assert out["joint_nis"][h] == (out["prefix_nis"][q][-1] if start[h + 1] > start[h] else 0.0)


def same_hypothesis(x, hx, y, hy, k=None):
    """Hypothesis hy of result y equals the first k pairings (all: None) of hypothesis hx of result x, bit for bit."""
    sx, sy = x["hyp_start"], y["hyp_start"]
    k = sy[hy + 1] - sy[hy] if k is None else k
    assert sy[hy + 1] - sy[hy] == k <= sx[hx + 1] - sx[hx]
    qx, qy = slice(sx[hx], sx[hx] + k), slice(sy[hy], sy[hy] + k)
    assert np.array_equal(x["prefix_nis"][qx], y["prefix_nis"][qy]), (hx, hy)
    assert np.array_equal(x["innovation"][qx], y["innovation"][qy]), (hx, hy)
    assert np.array_equal(x["innovation_cov"][hx][:k, :k], y["innovation_cov"][hy]), (hx, hy)
    if k == sx[hx + 1] - sx[hx]:
        assert x["joint_nis"][hx] == y["joint_nis"][hy]
    elif k > 0:
        assert y["joint_nis"][hy] == x["prefix_nis"][qx][-1]


def check_exact_rules(H, run):
    """The exact rules of bos_joint_compatibility, with run(start, pose, landmark, z, omega, batch=0) -> result:
    two calls, prefixes, the repeat, another order and company, and one hypothesis per batch."""
    full = run(*H.arrays())
    again = run(*H.arrays())
    n = len(H)
    for h in range(n):
        same_hypothesis(full, h, again, h)
    for k in PREFIXES:
        same_hypothesis(full, H.index["m32_one_pose"], full, H.index[f"prefix_{k}"], k)
    same_hypothesis(full, H.index["m32_random"], full, H.index["repeat"])
    order = list(reversed(range(n)))
    rev = run(*H.subset(order))
    for i, h in enumerate(order):
        same_hypothesis(full, h, rev, i)
    for h in (H.index["three_poses"], H.index["m32_one_pose"], H.index["fixed_pose"]):
        same_hypothesis(full, h, run(*H.subset([h])), 0)
    split = run(*H.arrays(), batch=1)
    for h in range(n):
        same_hypothesis(full, h, split, h)
    return full
