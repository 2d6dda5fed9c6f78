"""Reference, test bearings and checks shared by the bearing-association tests (host and GPU).

Quantities (bos.h bos_associate_bearings), for bearing q taken from pose a = pose[q] and landmark l:
  e_ref   = NumPy: arctan2 of the landmark in the pose's frame, minus z, wrapped to [-pi, pi)
  var_ref = the projected entry 0 of the pair (a, NP + l) from pair_cov_ref.PairReference: J Sigma_joint J^T
            over a dense inverse of the H the call linearised
  nis_ref = e_ref^2 / (var_ref + 1 / omega)
Bound: |nis - nis_ref| <= nis_ref (tol_var / S_ref + 64 eps), tol_var the bound pair_cov_ref.check_reference
applies to that pair's projected entry (2 tol s^2 with tol = n eps kappa_1(H_s), s = sum |J| sd). Entries
whose |e_ref| lies within WRAP_GUARD of pi are left out (a last-ulp difference flips the wrap there); they
may be at most WRAP_CAP of all entries.
Selection: a stable sort of the call's own nis_all row by (nis, stix), filtered by <= gate, non-finite
values dropped; compared exactly."""
import numpy as np

from helpers import EPS
from pair_cov_ref import PairReference

WRAP_GUARD = 1e-9
WRAP_CAP = 0.01
CAND_KEYS = ("cand_landmark", "cand_nis", "cand_innovation", "cand_var", "n_inside")


def predicted_bearings(pose_xyt, lm_xy, a):
    """[NL]: the bearing of every landmark in the frame of pose a."""
    x, y, th = pose_xyt[a]
    dx, dy = lm_xy[:, 0] - x, lm_xy[:, 1] - y
    c, s = np.cos(th), np.sin(th)
    return np.arctan2(-s * dx + c * dy, c * dx + s * dy)


def wrap(d):
    """[-pi, pi), by adding or subtracting 2 pi (exact where the result is small)."""
    d = np.array(d, dtype=np.float64)
    while np.any(d < -np.pi):
        d = np.where(d < -np.pi, d + 2 * np.pi, d)
    while np.any(d >= np.pi):
        d = np.where(d >= np.pi, d - 2 * np.pi, d)
    return d


def observed_landmark(P, a):
    """A landmark pose a observes (the first of its bearings), or a landmark by a's number where it observes none."""
    obs = P.b_lm[P.b_pose == a]
    return int(obs[0]) if len(obs) else int(a % P.NL)


def make_bearings(P, pose_xyt, lm_xy, poses):
    """(pose, z, omega) for the tests, four bearings per pose of `poses`: the prediction of a landmark the
    pose observes plus 0.01 rad; halfway between two landmarks' predictions; one whose innovation to a
    landmark is 0.03 rad short of pi, so the wrap matters; the first one again. omega is 1 and 25."""
    pose, z, omega = [], [], []
    for a in poses:
        pred = predicted_bearings(pose_xyt, lm_xy, a)
        l0 = observed_landmark(P, a)
        l1, l2, l3 = (l0 + 1) % P.NL, (l0 + 2) % P.NL, (l0 + 3) % P.NL
        za = [pred[l0] + 0.01, 0.5 * (pred[l1] + pred[l2]), pred[l3] - np.pi + 0.03, pred[l0] + 0.01]
        pose += [a] * 4
        z += za
        omega += [1.0, 25.0, 25.0, 1.0]
    return np.array(pose, dtype=np.int32), np.array(z), np.array(omega)


class AssocReference:
    """nis_ref [n, NL] with its bound and the excluded entries, for the bearings (pose, z, omega) of problem P
    against the lower triangle Hl of its H at the state (pose_xyt, lm_xy); dense: a shared DenseInverses."""

    def __init__(self, P, Hl, pose, z, omega, pose_xyt=None, lm_xy=None, dense=None):
        pose_xyt = P.pose_xyt if pose_xyt is None else pose_xyt
        lm_xy = P.lm_xy if lm_xy is None else lm_xy
        pose = np.asarray(pose)
        omega = np.ones(len(pose)) if omega is None else np.asarray(omega, dtype=np.float64)
        self.distinct = sorted(set(int(a) for a in pose))
        node_a = np.repeat(np.array(self.distinct, dtype=np.int32), P.NL)
        node_b = np.tile(P.NP + np.arange(P.NL, dtype=np.int32), len(self.distinct))
        self.pairs = PairReference(P, Hl, node_a, node_b, pose_xyt, lm_xy, dense=dense)
        self.node_a, self.node_b = node_a, node_b
        var = self.pairs.val["projected"][:, 0].reshape(len(self.distinct), P.NL)
        # check_reference asserts the projected entries' scaled error <= 2 tol: in absolute terms
        tol_var = (2 * self.pairs.tol * self.pairs.scale["projected"][:, 0]).reshape(len(self.distinct), P.NL)
        row = np.array([self.distinct.index(int(a)) for a in pose])
        self.var = var[row]                                                       # [n, NL]
        self.S = self.var + (1.0 / omega)[:, None]
        self.e = np.stack([wrap(predicted_bearings(pose_xyt, lm_xy, int(a)) - zq) for a, zq in zip(pose, z)])
        self.nis = self.e ** 2 / self.S
        self.bound = self.nis * (tol_var[row] / self.S + 64 * EPS)
        self.keep = np.abs(np.abs(self.e) - np.pi) > WRAP_GUARD
        self.excluded = float(1.0 - self.keep.mean())

    def check_var(self, projected_landmark_rows, label=""):
        """The variances themselves ([distinct poses, NL], the poses ascending) through check_reference."""
        proj = np.zeros((len(self.node_a), 9))
        proj[:, 0] = np.asarray(projected_landmark_rows).ravel()
        e = self.pairs.errors({"projected": proj, "cross": self.pairs.val["cross"], "cov_a": self.pairs.val["cov_a"],
                               "cov_b": self.pairs.val["cov_b"]})
        print(f"  association {label}: projected variances {e['projected']:.3g} of tol {self.pairs.tol:.3g}")
        assert e["projected"] <= 2 * self.pairs.tol
        return e["projected"]

    def check_nis(self, nis_all, label=""):
        """Prints the figures, then asserts the excluded share and the bound on every kept entry."""
        d = np.abs(nis_all - self.nis)
        with np.errstate(divide="ignore", invalid="ignore"):
            r = np.where(self.bound > 0, d / self.bound, np.where(d == 0, 0.0, np.inf))
        worst = float(r[self.keep].max())
        rel = float((d[self.keep] / np.maximum(self.nis[self.keep], 1e-300)).max())
        print(f"  association {label}: n {nis_all.shape} tol {self.pairs.tol:.3g} kappa_1 {self.pairs.kappa:.3g} excluded {self.excluded:.3g} "
              f"worst |nis - ref| / bound {worst:.3g} worst relative {rel:.3g}")
        assert self.excluded <= WRAP_CAP
        assert np.all(d[self.keep] <= self.bound[self.keep]), worst
        return worst


def expected_selection(row, gate, k):
    """(cand_landmark [k], cand_nis [k], n_inside) of one nis_all row."""
    idx = np.nonzero(np.isfinite(row) & (row <= gate))[0]
    order = idx[np.argsort(row[idx], kind="stable")][:k]     # idx ascends: equal NIS keep the lower stix first
    lm = np.full(k, -1, dtype=np.int32)
    nis = np.full(k, np.inf)
    lm[:len(order)] = order
    nis[:len(order)] = row[order]
    return lm, nis, len(idx)


def check_selection(out, gate, k):
    """cand_landmark, cand_nis and n_inside against the call's own nis_all, exactly; the padding; and
    cand_nis == cand_innovation^2 / cand_var in its bits."""
    rows = out["nis_all"]
    assert out["cand_landmark"].shape == (len(rows), k)
    for q, row in enumerate(rows):
        lm, nis, count = expected_selection(row, gate, k)
        assert np.array_equal(out["cand_landmark"][q], lm), (q, out["cand_landmark"][q], lm)
        assert np.array_equal(out["cand_nis"][q], nis), q
        assert out["n_inside"][q] == count, q
        listed = lm >= 0
        e, S = out["cand_innovation"][q], out["cand_var"][q]
        assert np.all(e[~listed] == 0.0) and np.all(S[~listed] == 0.0)
        assert np.array_equal(out["cand_nis"][q][listed], e[listed] ** 2 / S[listed]), q
