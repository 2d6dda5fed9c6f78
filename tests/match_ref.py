"""Reference, test measurements and checks shared by the node-matching tests (host and GPU).

Quantities (bos.h bos_match_landmarks / bos_match_poses), from pair_cov_ref.PairReference, a dense inverse of
the H the call linearised:
  landmark query a against landmark l: C_ref = the projected block of the pair (NP + a, NP + l), d_ref = l_a - l_l,
                                       d2_ref = d^T C_ref^-1 d
  pose a, measurement (z, Omega), against pose u: P_ref = the projected block of the pair (a, u),
                                       S_ref = P_ref + np.linalg.inv(Omega), e_ref in NumPy (the odometry error of
                                       (a, u, z), its angle wrapped to [-pi, pi)), nis_ref = e^T S_ref^-1 e
Bound, with M = C_ref or S_ref, v = d or e and y = M^-1 v:
  |score - score_ref| <= 2 |y|_1^2 tol_M + 4 |y|_1 dv + 64 eps score_ref
tol_M the largest absolute bound pair_cov_ref.check_reference puts on that pair's projected entries
(2 tol scale), dv = 64 eps (1 + |t_u - t_a| + |z|) for poses and 64 eps (|l_a| + |l_l|) for landmarks. The first
term is the first-order change y^T dM y of the score, doubled for the second-order remainder: valid while
tol_M |M^-1|_2 <= 0.1, asserted on the reference alone (check_condition).
Left out: the landmark entry l == a (NaN by definition, checked as such), and pose entries whose |e_ref[2]|
lies within WRAP_GUARD of pi (at most WRAP_CAP of all entries).
Selection: a stable sort of the call's own row by (score, stix), filtered by <= gate, non-finite values
dropped; compared exactly (associate_ref.expected_selection)."""
import numpy as np

from associate_ref import WRAP_CAP, WRAP_GUARD, expected_selection, wrap
from helpers import EPS
from pair_cov_ref import PairReference

LM_KEYS = ("cand_landmark", "cand_d2", "cand_diff", "cand_cov", "n_inside", "d2_all")
POSE_KEYS = ("cand_pose", "cand_nis", "cand_innovation", "cand_cov", "n_inside", "nis_all")
OMEGAS = {"diag": np.diag([500.0, 500.0, 5000.0]),
          "full": np.array([[400.0, 30.0, -20.0], [30.0, 300.0, 50.0], [-20.0, 50.0, 2000.0]]),
          "identity": np.eye(3)}
CONDITION_CAP = 0.1


def query_landmarks(P):
    """The first, a middle and the last landmark."""
    return sorted({0, P.NL // 2, P.NL - 1})


def query_poses(P):
    """The fixed pose, the first and the last pose."""
    return sorted({P.fixed, 0, P.NP - 1})


def predicted_odometry(pose_xyt, a):
    """[NP, 3]: the prediction of every pose in the frame of pose a (angle wrapped to [-pi, pi))."""
    x, y, th = pose_xyt[a]
    dx, dy = pose_xyt[:, 0] - x, pose_xyt[:, 1] - y
    c, s = np.cos(th), np.sin(th)
    return np.stack([c * dx + s * dy, -s * dx + c * dy, wrap(pose_xyt[:, 2] - th)], axis=1)


def make_measurements(P, pose_xyt, poses):
    """(pose, z [n, 3], omega [n, 9]) for the tests, four measurements per pose of `poses`: the prediction
    toward a chosen pose plus a small offset (Omega diagonal); toward another one (a full SPD Omega); one whose
    angle error toward a third is 0.03 rad short of the wrap (the identity); the first one again."""
    pose, z, omega = [], [], []
    for a in poses:
        pred = predicted_odometry(pose_xyt, a)
        u0, u1, u2 = (a + 3) % P.NP, (a + P.NP // 2) % P.NP, (a + 1) % P.NP
        first = pred[u0] + np.array([0.02, -0.01, 0.004])
        za = [first, pred[u1] + np.array([-0.05, 0.03, -0.01]), pred[u2] - np.array([0.01, 0.0, np.pi - 0.03]), first]
        pose += [a] * 4
        z += za
        omega += [OMEGAS["diag"].ravel(), OMEGAS["full"].ravel(), OMEGAS["identity"].ravel(), OMEGAS["diag"].ravel()]
    return np.array(pose, dtype=np.int32), np.array(z), np.array(omega)


def solve_rows(M, v):
    """y = M^-1 v and |M^-1|_2 for stacks [..., d, d], [..., d]; singular entries give inf."""
    y = np.full(v.shape, np.inf)
    inv2 = np.full(v.shape[:-1], np.inf)
    for i in np.ndindex(*v.shape[:-1]):
        w = np.linalg.eigvalsh(M[i])
        if w[0] > 0:
            y[i] = np.linalg.solve(M[i], v[i])
            inv2[i] = 1.0 / w[0]
    return y, inv2


class _ScoreReference:
    """score [n, N] with its bound, keep [n, N] and the figures the checks print; built by the two
    subclasses from M [n, N, d, d], v [n, N, d], tol_M [n, N] and dv [n, N]."""

    def _finish(self, M, v, tol_M, dv, keep):
        y, inv2 = solve_rows(M, v)
        self.M, self.v, self.keep = M, v, keep
        with np.errstate(invalid="ignore"):
            self.score = np.einsum("...i,...i->...", v, y)
            y1 = np.abs(y).sum(axis=-1)
            self.bound = 2 * y1 ** 2 * tol_M + 4 * y1 * dv + 64 * EPS * self.score
            self.condition = float((tol_M * inv2)[keep].max())
        self.excluded = float(1.0 - keep.mean())

    def check_condition(self, label=""):
        print(f"  matching reference {label}: tol {self.pairs.tol:.3g} kappa_1 {self.pairs.kappa:.3g} worst tol_M |M^-1|_2 "
              f"{self.condition:.3g} excluded {self.excluded:.3g}")
        assert self.condition <= CONDITION_CAP

    def check_scores(self, rows, label="", bound=None):
        """Prints the figures, then asserts the bound on every kept entry; returns the worst share of it."""
        bound = self.bound if bound is None else bound
        k = self.keep
        d = np.abs(rows - self.score)
        assert np.isfinite(rows[k]).all()
        worst = float((d[k] / np.maximum(bound[k], 1e-300)).max())
        rel = float((d[k] / np.maximum(self.score[k], 1e-300)).max())
        print(f"  matching {label}: rows {rows.shape} worst |score - ref| / bound {worst:.3g} worst relative {rel:.3g} "
              f"worst relative bound {float((bound[k] / np.maximum(self.score[k], 1e-300)).max()):.3g}")
        assert np.all(d[k] <= bound[k]), worst
        return worst


class LandmarkReference(_ScoreReference):
    """d2_ref [n, NL] of the query landmarks against the lower triangle Hl of P's H at (pose_xyt, lm_xy)."""

    def __init__(self, P, Hl, landmarks, pose_xyt=None, lm_xy=None, dense=None):
        pose_xyt = P.pose_xyt if pose_xyt is None else pose_xyt
        lm_xy = P.lm_xy if lm_xy is None else lm_xy
        landmarks = np.asarray(landmarks)
        self.distinct = sorted(set(int(a) for a in landmarks))
        node_a = np.repeat(P.NP + np.array(self.distinct, dtype=np.int32), P.NL)
        node_b = np.tile(P.NP + np.arange(P.NL, dtype=np.int32), len(self.distinct))
        self.pairs = PairReference(P, Hl, node_a, node_b, pose_xyt, lm_xy, dense=dense)
        shape = (len(self.distinct), P.NL)
        C = self.pairs.val["projected"][:, :4].reshape(*shape, 2, 2)
        tol = (2 * self.pairs.tol * self.pairs.scale["projected"][:, :4]).max(axis=1).reshape(shape)
        row = np.array([self.distinct.index(int(a)) for a in landmarks])
        la = lm_xy[landmarks]                                                         # [n, 2]
        v = la[:, None, :] - lm_xy[None, :, :]
        dv = 64 * EPS * (np.linalg.norm(la, axis=1)[:, None] + np.linalg.norm(lm_xy, axis=1)[None, :])
        keep = np.arange(P.NL)[None, :] != landmarks[:, None]
        self._finish(C[row].astype(np.float64), v, tol[row].astype(np.float64), dv, keep)


class PoseReference(_ScoreReference):
    """nis_ref [n, NP] of the measurements (pose, z, omega [n, 9]) against Hl at (pose_xyt, lm_xy)."""

    def __init__(self, P, Hl, pose, z, omega, pose_xyt=None, lm_xy=None, dense=None):
        pose_xyt = P.pose_xyt if pose_xyt is None else pose_xyt
        lm_xy = P.lm_xy if lm_xy is None else lm_xy
        pose, z = np.asarray(pose), np.asarray(z, dtype=np.float64).reshape(-1, 3)
        omega = np.tile(np.eye(3).ravel(), (len(pose), 1)) if omega is None else np.asarray(omega, dtype=np.float64).reshape(-1, 9)
        self.distinct = sorted(set(int(a) for a in pose))
        node_a = np.repeat(np.array(self.distinct, dtype=np.int32), P.NP)
        node_b = np.tile(np.arange(P.NP, dtype=np.int32), len(self.distinct))
        self.pairs = PairReference(P, Hl, node_a, node_b, pose_xyt, lm_xy, dense=dense)
        shape = (len(self.distinct), P.NP)
        Pm = self.pairs.val["projected"].reshape(*shape, 3, 3)
        tol = (2 * self.pairs.tol * self.pairs.scale["projected"]).max(axis=1).reshape(shape)
        row = np.array([self.distinct.index(int(a)) for a in pose])
        R = np.stack([np.linalg.inv(o.reshape(3, 3)) for o in omega])
        M = Pm[row].astype(np.float64) + R[:, None, :, :]
        pred = np.stack([predicted_odometry(pose_xyt, int(a)) for a in pose])        # [n, NP, 3]
        v = pred - z[:, None, :]
        v[:, :, 2] = wrap(v[:, :, 2])
        dist = np.linalg.norm(pose_xyt[None, :, :2] - pose_xyt[pose][:, None, :2], axis=2)
        dv = 64 * EPS * (1 + dist + np.linalg.norm(z, axis=1)[:, None])
        keep = np.abs(np.abs(v[:, :, 2]) - np.pi) > WRAP_GUARD
        self._finish(M, v, tol[row].astype(np.float64), dv, keep)
        self.e = v

    def check_condition(self, label=""):
        super().check_condition(label)
        assert self.excluded <= WRAP_CAP


def landmark_recipe(d, C):
    """d2 from d [2] and C [4] in NumPy scalar fp64 arithmetic, by the recipe of bos.h."""
    d0, d1 = np.float64(d[0]), np.float64(d[1])
    c00, c10, c11 = np.float64(C[0]), np.float64(C[2]), np.float64(C[3])
    D0 = c00
    if not (np.isfinite(D0) and D0 > 0):
        return np.float64(np.nan)
    t = c10 / D0
    D1 = c11 - t * c10
    if not (np.isfinite(D1) and D1 > 0):
        return np.float64(np.nan)
    y1 = d1 - t * d0
    return (d0 * d0) / D0 + (y1 * y1) / D1


def pose_recipe(e, S):
    """nis from e [3] and S [9] (its lower triangle) in NumPy scalar fp64 arithmetic, by the recipe of bos.h."""
    e0, e1, e2 = (np.float64(x) for x in e)
    s00, s10, s11, s20, s21, s22 = (np.float64(S[i]) for i in (0, 3, 4, 6, 7, 8))
    D0 = s00
    if not (np.isfinite(D0) and D0 > 0):
        return np.float64(np.nan)
    l10 = s10 / D0
    l20 = s20 / D0
    D1 = s11 - l10 * s10
    if not (np.isfinite(D1) and D1 > 0):
        return np.float64(np.nan)
    t21 = s21 - l20 * s10
    l21 = t21 / D1
    D2 = (s22 - l20 * s20) - l21 * t21
    if not (np.isfinite(D2) and D2 > 0):
        return np.float64(np.nan)
    y0 = e0
    y1 = e1 - l10 * y0
    y2 = (e2 - l20 * y0) - l21 * y1
    return ((y0 * y0) / D0 + (y1 * y1) / D1) + (y2 * y2) / D2


def check_selection(out, keys, gate, k, recipe):
    """The lists and counts against the call's own rows, exactly; the padding; every listed score
    reproduced bit for bit from its listed details by `recipe`."""
    ix, score, detail, cov, count, rows = (out[key] for key in keys)
    assert ix.shape == (len(rows), k)
    for q, row in enumerate(rows):
        want_ix, want_score, want_count = expected_selection(row, gate, k)
        assert np.array_equal(ix[q], want_ix), (q, ix[q], want_ix)
        assert np.array_equal(score[q], want_score), q
        assert count[q] == want_count, q
        listed = want_ix >= 0
        assert np.all(detail[q][~listed] == 0.0) and np.all(cov[q][~listed] == 0.0)
        with np.errstate(all="ignore"):
            again = np.array([recipe(detail[q][j], cov[q][j]) for j in np.nonzero(listed)[0]])
        assert np.array_equal(score[q][listed], again), (q, score[q][listed], again)


def check_landmark_selection(out, gate, k):
    check_selection(out, LM_KEYS, gate, k, landmark_recipe)


def check_pose_selection(out, gate, k):
    check_selection(out, POSE_KEYS, gate, k, pose_recipe)
    S = out["cand_cov"].reshape(-1, 3, 3)
    assert np.array_equal(S, S.transpose(0, 2, 1))                                   # mirrored
