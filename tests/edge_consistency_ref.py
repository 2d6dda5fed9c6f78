"""Reference and checks shared by the edge-consistency tests (host and GPU), on top of edge_cov_ref.EdgeReference:
a dense inverse of the system the call itself linearised.

Quantities (bos.h bos_edge_consistency), NumPy on the oracle's residuals:
  bearing i:   e_ref = the oracle's bearing error (oracle.bearing_errors)
               T_ref = 1 / omega - var_ref,  w2_ref = e_ref^2 / T_ref
  odometry j:  e_ref = the oracle's odometry error (oracle.odometry_error_and_jacobian)
               T_ref = inv(Omega) - P_ref,   w2_ref = e_ref . solve(T_ref, e_ref)
The bound below is first order in the covariance's error alone: it leaves no room for a residual that rounds
differently, and the datasets hold residuals AT rounding level (a landmark triangulated from two bearings, a pose
integrated from its odometry edge: e is 0 or a few 1e-16 at the initial guess), where an arctan2 that differs in its
last bit changes w2 by a factor. The oracle's error code is independent of the product's and was written to round
as it does (the portable atan2, the explicit fma), so e_ref carries no rounding of its own into the comparison.
var_ref / P_ref are EdgeReference's bearing_var / odom_cov. edge_cov_ref.check_reference grants a projected entry
the error 2 tol scale (tol = n eps kappa_1(H_s)); in absolute terms tol_var = 2 tol bearing_var_scale and the
matrix tol_P = 2 tol odom_cov_scale. To first order in that error
  |w2 - w2_ref| <= w2_ref (delta + 64 eps),  delta = tol_var / T_ref             (bearing)
                                             delta = ||T_ref^-1||_2 ||tol_P||_2   (odometry).
Left out: entries with delta >= 1/2 (or T_ref not positive definite): the edge has almost no redundancy and T is a
cancellation no arithmetic can save; entries with |e_ref| (the angle) within associate_ref.WRAP_GUARD of pi; and
odometry self-loops, whose w2 and redundancy must be NaN. The first two together may be at most
associate_ref.WRAP_CAP of a kind's edges, of both kinds in every world check_rows is given. C1 as it is distributed
does not meet that, by the reference alone: its odometry's information (500, 500, 5000) against bearings of
information 1 leaves an odometry edge a redundancy of about 0.01 (1.5e-5 at the least), T is a cancellation of R
against P and delta >= 1/2 for 87 % of its odometry edges (34 % in its edge-case world). The accuracy tests
therefore run on C1 with the odometry's information divided by 100 (test_edge_consistency_host.soft_odometry_world:
redundancy about 0.14, no odometry edge excluded at the initial guess, after convergence or in its edge-case world).
The same per-edge errors bound tr(Omega P): omega tol_var for a bearing, sum |Omega_ab| tol_P_ab for an odometry
edge; they give the allowance of the trace identity and of the redundancy's range, with no further tolerance.
Lists and counts: a stable sort of the call's own rows, compared exactly, the padding included, and the listed w2
replayed from the listed e and T in its bits."""
import numpy as np

import oracle as O
from associate_ref import WRAP_CAP, WRAP_GUARD
from edge_cov_ref import EdgeReference
from helpers import EPS, to_oracle

LIST_KEYS = ("cand_bearing", "cand_bearing_w2", "cand_bearing_innovation", "cand_bearing_resvar", "n_over_bearing",
             "cand_odom", "cand_odom_w2", "cand_odom_innovation", "cand_odom_rescov", "n_over_odom")
ROW_KEYS = ("bearing_w2", "bearing_chi2", "bearing_redundancy", "odom_w2", "odom_chi2", "odom_redundancy")


class ConsistencyReference:
    """w2_ref, chi2_ref and tr(Omega P)_ref of every edge of P with their bounds and the excluded entries, over the
    lower triangle Hl of the H the call linearised, at the state (pose_xyt, lm_xy) (P's own unless given)."""

    def __init__(self, P, Hl, pose_xyt=None, lm_xy=None):
        pose = P.pose_xyt if pose_xyt is None else pose_xyt
        lm = P.lm_xy if lm_xy is None else lm_xy
        self.P = P
        self.edges = ref = EdgeReference(P, Hl, pose, lm)
        self.tol = ref.tol
        Mb, Mo = len(P.b_z), len(P.o_z)
        # ---- bearings
        self.b_e = O.bearing_errors(to_oracle(P), pose, lm) if Mb else np.zeros(0)
        om = np.ones(Mb) if P.b_omega is None else P.b_omega
        self.b_omega = om
        self.b_T = 1.0 / om - ref.bearing_var
        tol_var = 2 * ref.tol * ref.bearing_var_scale
        with np.errstate(divide="ignore", invalid="ignore"):
            self.b_w2 = self.b_e ** 2 / self.b_T
            self.b_delta = np.where(self.b_T > 0, tol_var / self.b_T, np.inf)
        self.b_chi2 = self.b_e * om * self.b_e
        self.b_trace, self.b_trace_tol = om * ref.bearing_var, om * tol_var
        self.b_cancel = ~(self.b_delta < 0.5)
        self.b_wrap = np.abs(np.abs(self.b_e) - np.pi) <= WRAP_GUARD
        self.b_keep = ~(self.b_cancel | self.b_wrap)
        # ---- odometry
        self.o_e = (np.stack([O.odometry_error_and_jacobian(pose[a], pose[d], z)[0] for a, d, z in zip(P.o_src, P.o_dst, P.o_z)])
                    if Mo else np.zeros((0, 3)))
        Om = P.o_omega.reshape(Mo, 3, 3)
        self.o_loop = P.o_src == P.o_dst
        self.o_T = (np.linalg.inv(Om) if Mo else np.zeros((0, 3, 3))) - ref.odom_cov
        tol_P = 2 * ref.tol * ref.odom_cov_scale
        self.o_w2, self.o_delta = np.full(Mo, np.nan), np.full(Mo, np.inf)
        for j in range(Mo):
            T = 0.5 * (self.o_T[j] + self.o_T[j].T)
            if self.o_loop[j] or not np.all(np.linalg.eigvalsh(T) > 0):
                continue
            self.o_w2[j] = float(self.o_e[j] @ np.linalg.solve(T, self.o_e[j]))
            self.o_delta[j] = np.linalg.norm(np.linalg.inv(T), 2) * np.linalg.norm(tol_P[j], 2)
        self.o_chi2 = np.einsum("mi,mij,mj->m", self.o_e, Om, self.o_e)
        self.o_trace = np.einsum("mij,mij->m", Om, ref.odom_cov)
        self.o_trace_tol = np.einsum("mij,mij->m", np.abs(Om), tol_P)
        self.o_cancel = ~(self.o_delta < 0.5) & ~self.o_loop
        self.o_wrap = (np.abs(np.abs(self.o_e[:, 2]) - np.pi) <= WRAP_GUARD) & ~self.o_loop
        self.o_keep = ~(self.o_cancel | self.o_wrap | self.o_loop)
        self.excluded = {"bearing": float(1.0 - self.b_keep.mean()) if Mb else 0.0,
                         "odom": float((self.o_cancel | self.o_wrap).mean()) if Mo else 0.0}

    def check_rows(self, out, label=""):
        """Prints the figures, then asserts the excluded share of each kind and the bound on every kept w2; chi2 within 64 eps of
        its scale; a self-loop's w2 and redundancy NaN; the redundancy's range. Returns the worst ratio to the bound."""
        worst = 0.0
        for kind, w2, ref, delta, keep in (("bearing", out["bearing_w2"], self.b_w2, self.b_delta, self.b_keep),
                                           ("odom", out["odom_w2"], self.o_w2, self.o_delta, self.o_keep)):
            if not len(w2):
                continue
            bound = ref[keep] * (delta[keep] + 64 * EPS)
            d = np.abs(w2[keep] - ref[keep])
            with np.errstate(divide="ignore", invalid="ignore"):
                r = np.where(bound > 0, d / bound, np.where(d == 0, 0.0, np.inf))
            ratio = float(r.max()) if len(r) else 0.0
            cancel, wraps = (self.b_cancel, self.b_wrap) if kind == "bearing" else (self.o_cancel, self.o_wrap)
            print(f"  edge consistency {label} {kind}: edges {len(w2)} tol {self.tol:.3g} excluded {self.excluded[kind]:.3g} "
                  f"(cancellation {int(cancel.sum())}, wrap {int(wraps.sum())}) "
                  f"largest delta kept {float(delta[keep].max()) if keep.any() else 0.0:.3g} worst |w2 - ref| / bound {ratio:.3g} "
                  f"largest w2 {float(np.nanmax(w2)):.3g}")
            assert self.excluded[kind] <= WRAP_CAP, (kind, self.excluded[kind])
            assert np.all(np.isfinite(w2[keep])), kind
            assert np.all(d <= bound), (kind, ratio)
            worst = max(worst, ratio)
        # chi2: no covariance involved. |e - e_ref| is a few ulps of the angles and coordinates the error is the
        # difference of (at most 4 pi, the coordinates' span): 64 eps of that scale in e, to first order in chi2
        bw = ~self.b_wrap
        span = 4 * np.pi + 2 * float(np.abs(self.P.pose_xyt[:, :2]).max())
        assert np.all(np.abs(out["bearing_chi2"] - self.b_chi2)[bw] <=
                      64 * EPS * (self.b_chi2 + 2 * self.b_omega * np.abs(self.b_e) * 4 * np.pi + 1e-300)[bw])
        if len(out["odom_chi2"]):
            ow = np.abs(np.abs(self.o_e[:, 2]) - np.pi) > WRAP_GUARD
            Om = np.abs(self.P.o_omega.reshape(-1, 3, 3))
            slack = 64 * EPS * (self.o_chi2 + 2 * span * np.einsum("mi,mij->m", np.abs(self.o_e), Om))
            assert np.all(np.abs(out["odom_chi2"] - self.o_chi2)[ow] <= slack[ow] + 1e-300)
        assert np.all(np.isnan(out["odom_w2"][self.o_loop])) and np.all(np.isnan(out["odom_redundancy"][self.o_loop]))
        assert np.all(np.isfinite(out["odom_chi2"]))
        # redundancy in [0, 1] up to the projected entries' granted error
        rb, ro = out["bearing_redundancy"], out["odom_redundancy"][~self.o_loop]
        assert np.all(rb >= -self.b_trace_tol - 64 * EPS) and np.all(rb <= 1 + self.b_trace_tol + 64 * EPS)
        ot = self.o_trace_tol[~self.o_loop] / 3
        assert np.all(ro >= -ot - 64 * EPS) and np.all(ro <= 1 + ot + 64 * EPS)
        return worst

    def check_trace(self, out, n, damping, pose_cov, lm_cov, label=""):
        """sum tr(Omega P) = n - lambda tr(Sigma) on the call's fp64 values (self-loops skipped). The allowance is
        the sum of the per-edge bounds of tr(Omega P) plus what marginals_ref.Reference grants the diagonal of
        Sigma (tol Sigma_ii each) times lambda, plus the sums' own rounding, 64 eps of n."""
        lhs = float(np.sum(1.0 - out["bearing_redundancy"]) + 3.0 * np.nansum(1.0 - out["odom_redundancy"]))
        tr = float(np.trace(pose_cov, axis1=1, axis2=2).sum() + (np.trace(lm_cov, axis1=1, axis2=2).sum() if len(lm_cov) else 0.0))
        rhs = n - damping * tr
        allow = float(self.b_trace_tol.sum() + self.o_trace_tol[~self.o_loop].sum() + damping * self.tol * tr + 64 * EPS * n)
        print(f"  edge consistency {label} trace identity: sum tr(Omega P) {lhs:.12g} n - lambda tr(Sigma) {rhs:.12g} "
              f"difference {abs(lhs - rhs):.3g} allowance {allow:.3g}")
        assert abs(lhs - rhs) <= allow


def expected_list(w2, gate, k):
    """(edge index [k], w2 [k], n_over) of one row: the k largest finite w2 >= gate, equal ones to the lower index first."""
    idx = np.nonzero(np.isfinite(w2) & (w2 >= gate))[0]
    order = idx[np.argsort(-w2[idx], kind="stable")][:k]
    ix, val = np.full(k, -1, dtype=np.int32), np.full(k, -np.inf)
    ix[:len(order)] = order
    val[:len(order)] = w2[order]
    return ix, val, len(idx)


def replay_odom_w2(e, T):
    """bos.h's LDL^T sequence on one listed odometry edge, float64 scalars (no contraction)."""
    e = [np.float64(v) for v in e]
    s00, s10, s11, s20, s21, s22 = (np.float64(T[a][b]) for a, b in ((0, 0), (1, 0), (1, 1), (2, 0), (2, 1), (2, 2)))
    D0 = s00
    l10, l20 = s10 / D0, s20 / D0
    D1 = s11 - l10 * s10
    t21 = s21 - l20 * s10
    l21 = t21 / D1
    D2 = (s22 - l20 * s20) - l21 * t21
    y0 = e[0]
    y1 = e[1] - l10 * y0
    y2 = (e[2] - l20 * y0) - l21 * y1
    return ((y0 * y0) / D0 + (y1 * y1) / D1) + (y2 * y2) / D2


def check_lists(out, gate_bearing, gate_odom, k):
    """The lists and counts against the call's own rows, exactly, with the padding; cand_w2 from e and T in its bits."""
    for kind, gate in (("bearing", gate_bearing), ("odom", gate_odom)):
        w2 = out[f"{kind}_w2"]
        ix, val, count = expected_list(w2, gate, k)
        cand, cw = out[f"cand_{kind}"], out[f"cand_{kind}_w2"]
        e = out[f"cand_{kind}_innovation"]
        T = out["cand_bearing_resvar" if kind == "bearing" else "cand_odom_rescov"]
        assert cand.shape == (k,)
        assert np.array_equal(cand, ix), (kind, cand, ix)
        assert np.array_equal(cw, val), (kind, cw, val)
        assert out[f"n_over_{kind}"] == count, kind
        listed = ix >= 0
        assert np.all(e[~listed] == 0.0) and np.all(T[~listed] == 0.0)
        if kind == "bearing":
            assert np.array_equal(cw[listed], e[listed] ** 2 / T[listed])
        else:
            assert np.array_equal(T, T.transpose(0, 2, 1))
            for j in np.nonzero(listed)[0]:
                assert cw[j] == replay_odom_w2(e[j], T[j]), (j, cw[j])
