"""Reference and error measures shared by the edge-covariance tests (host and GPU), built on
marginals_ref.Reference.

Reference: Sigma_ref = inv(H), H the symmetrised H_nf without the fixed pose, dense fp64, padded with
zeros for the fixed pose; an edge's cross block and Sigma_joint are read out of it. J_ref is this
module's own NumPy restatement of the two Jacobians of csrc/host/bos_math.hpp (g = R^T (l - t) and the
columns as written there), at the state the caller gives.

Error of a cross entry (i, j): |out - ref| / sqrt(Sigma_ref[i, i] Sigma_ref[j, j]) <= tol, the
marginals' own measure and bound tol = n eps kappa_1(H_s).
Error of a projected entry (u, v): |out - ref| / (s_u s_v), s_u = sum_i |J_ui| sd_i with
sd_i = sqrt(Sigma_ref[i, i]), <= 2 tol: every entry of Sigma_joint is off by at most tol sd_i sd_j, so
the bilinear form is off by at most tol s_u s_v; the second tol covers the Jacobians' own rounding (a
few eps relative, below tol >= n eps) and the sum's.
Where a scale is zero (only the fixed pose's dofs are involved) the output must be exactly zero.

RefinedEdgeReference / check_refined add the refined criterion of marginals_ref.py to the three groups:
the same measures against Sigma* (refined in np.longdouble; J of the projection in longdouble too), each
group within 8 x the larger error of two plain fp64 inverses of the same H over the same entries."""
import numpy as np

from marginals_ref import MARGIN, DenseInverses, Reference, RefinedBlocks, ratio


def bearing_jacobians(pose, lm):
    """[M, 5] = [d/dt_x, d/dt_y, d/dtheta, d/dl_x, d/dl_y] of the bearing of lm [M, 2] from pose [M, 3]."""
    c, s = np.cos(pose[:, 2]), np.sin(pose[:, 2])
    dx, dy = lm[:, 0] - pose[:, 0], lm[:, 1] - pose[:, 1]
    gx, gy = c * dx + s * dy, -s * dx + c * dy          # g = R^T (l - t)
    f = 1.0 / (gx * gx + gy * gy)
    a0, a1 = -f * gy, f * gx                             # d atan2(g) / dg
    lx, ly = lm[:, 0], lm[:, 1]
    J = np.zeros((len(pose), 5), dtype=pose.dtype)
    J[:, 3] = a0 * c - a1 * s                            # a R^T
    J[:, 4] = a0 * s + a1 * c
    J[:, 0], J[:, 1] = -J[:, 3], -J[:, 4]
    J[:, 2] = a0 * (c * ly - s * lx) + a1 * (-s * ly - c * lx)   # a R^T [[0, 1], [-1, 0]] l
    return J


def odometry_jacobians(src, dst):
    """[M, 3, 6] over [dx_s, dy_s, dth_s, dx_d, dy_d, dth_d] of the odometry prediction src -> dst."""
    c, s = np.cos(src[:, 2]), np.sin(src[:, 2])
    xd, yd = dst[:, 0], dst[:, 1]
    J = np.zeros((len(src), 3, 6), dtype=src.dtype)
    J[:, 0, 0], J[:, 0, 1], J[:, 0, 2] = -c, -s, -s * xd + c * yd
    J[:, 0, 3], J[:, 0, 4], J[:, 0, 5] = c, s, s * xd - c * yd
    J[:, 1, 0], J[:, 1, 1], J[:, 1, 2] = s, -c, -c * xd - s * yd
    J[:, 1, 3], J[:, 1, 4], J[:, 1, 5] = -s, c, s * yd + c * xd
    J[:, 2, 2], J[:, 2, 5] = -1.0, 1.0
    return J


class EdgeReference(Reference):
    """Reference plus every edge's cross block, projected covariance and their scales, for the
    problem P, the lower triangle Hl of its H (reference dof numbering) and the state J is taken at
    (P's own unless given)."""

    def __init__(self, P, Hl, pose_xyt=None, lm_xy=None, dense=None):
        super().__init__(P, Hl, dense=dense)
        if dense is None:
            Hd = Hl.toarray()
            H = (Hd + np.tril(Hd, -1).T)[np.ix_(self.idx, self.idx)]
            S = np.linalg.inv(H)
        else:
            S = dense.lu
        full = np.zeros((P.N, P.N))
        full[np.ix_(self.idx, self.idx)] = S
        self.full = full
        sd = np.sqrt(np.diag(full))
        pose = P.pose_xyt if pose_xyt is None else pose_xyt
        lm = P.lm_xy if lm_xy is None else lm_xy
        three, two = np.arange(3), np.arange(2)
        bp = 3 * P.b_pose.astype(np.int64)[:, None] + three
        bl = 3 * P.NP + 2 * P.b_lm.astype(np.int64)[:, None] + two
        oa = 3 * P.o_src.astype(np.int64)[:, None] + three
        ob = 3 * P.o_dst.astype(np.int64)[:, None] + three
        self.bearing_cross = full[bp[:, :, None], bl[:, None, :]]
        self.odom_cross = full[oa[:, :, None], ob[:, None, :]]
        self.bearing_cross_scale = sd[bp][:, :, None] * sd[bl][:, None, :]
        self.odom_cross_scale = sd[oa][:, :, None] * sd[ob][:, None, :]
        bi, oi = np.concatenate([bp, bl], axis=1), np.concatenate([oa, ob], axis=1)
        Jb = bearing_jacobians(pose[P.b_pose], lm[P.b_lm])
        Jo = odometry_jacobians(pose[P.o_src], pose[P.o_dst])
        self.bearing_var = np.einsum("mi,mij,mj->m", Jb, full[bi[:, :, None], bi[:, None, :]], Jb)
        self.odom_cov = np.einsum("mui,mij,mvj->muv", Jo, full[oi[:, :, None], oi[:, None, :]], Jo)
        self.bearing_var_scale = (np.abs(Jb) * sd[bi]).sum(axis=1) ** 2
        so = (np.abs(Jo) * sd[oi][:, None, :]).sum(axis=2)
        self.odom_cov_scale = so[:, :, None] * so[:, None, :]

    @staticmethod
    def _scaled(out, ref, scale):
        if out.size == 0:
            return 0.0
        zero = scale == 0.0
        assert np.all(out[zero] == 0.0), "an entry of the fixed pose alone is not exactly zero"
        return float((np.abs(out - ref)[~zero] / scale[~zero]).max()) if (~zero).any() else 0.0

    def cross_error(self, bearing_cross, odom_cross):
        return max(self._scaled(bearing_cross, self.bearing_cross, self.bearing_cross_scale),
                   self._scaled(odom_cross, self.odom_cross, self.odom_cross_scale))

    def projected_error(self, bearing_var, odom_cov):
        return max(self._scaled(bearing_var, self.bearing_var, self.bearing_var_scale),
                   self._scaled(odom_cov, self.odom_cov, self.odom_cov_scale))


def edge_entries(P, full, pose, lm):
    """Every edge's cross block and projected covariance out of a padded N x N matrix `full`, the
    Jacobians evaluated in full's dtype at the state (pose, lm). Returns (entries dict, Jb, Jo, bi, oi)."""
    three, two = np.arange(3), np.arange(2)
    bp = 3 * P.b_pose.astype(np.int64)[:, None] + three
    bl = 3 * P.NP + 2 * P.b_lm.astype(np.int64)[:, None] + two
    oa = 3 * P.o_src.astype(np.int64)[:, None] + three
    ob = 3 * P.o_dst.astype(np.int64)[:, None] + three
    bi, oi = np.concatenate([bp, bl], axis=1), np.concatenate([oa, ob], axis=1)
    pose, lm = pose.astype(full.dtype), lm.astype(full.dtype)
    Jb = bearing_jacobians(pose[P.b_pose], lm[P.b_lm])
    Jo = odometry_jacobians(pose[P.o_src], pose[P.o_dst])
    ent = {"bearing_cross": full[bp[:, :, None], bl[:, None, :]], "odom_cross": full[oa[:, :, None], ob[:, None, :]],
           "bearing_var": np.einsum("mi,mij,mj->m", Jb, full[bi[:, :, None], bi[:, None, :]], Jb),
           "odom_cov": np.einsum("mui,mij,mvj->muv", Jo, full[oi[:, :, None], oi[:, None, :]], Jo)}
    return ent, Jb, Jo, bi, oi


class RefinedEdgeReference(EdgeReference):
    """EdgeReference (the old bounds' Sigma_ref and tol, unchanged) plus the refined criterion of
    marginals_ref.py for the blocks, the cross blocks and the projected covariances. Sigma* gives the
    reference values and the scales (the Jacobians of the projection in np.longdouble); e_ref of each
    group is the larger error of the two plain fp64 inverses (LU, Cholesky) over the same entries, their
    projections formed in fp64. .e_ref / .e_lu / .e_chol: dicts over "blocks", "cross", "projected"."""

    KEYS = {"cross": ("bearing_cross", "odom_cross"), "projected": ("bearing_var", "odom_cov")}

    def __init__(self, P, Hl, pose_xyt=None, lm_xy=None):
        d = DenseInverses(P, Hl)
        super().__init__(P, Hl, pose_xyt, lm_xy, dense=d)
        pose = P.pose_xyt if pose_xyt is None else pose_xyt
        lm = P.lm_xy if lm_xy is None else lm_xy
        self.residual = d.residual
        star_full = d.full(d.star)
        self.refined = RefinedBlocks(P, d, star_full)
        sd = self.refined.sd
        self.star, Jb, Jo, bi, oi = edge_entries(P, star_full, pose, lm)
        three, two = slice(0, 3), slice(3, 5)
        so = (np.abs(Jo) * sd[oi][:, None, :]).sum(axis=2)
        self.star_scale = {"bearing_cross": sd[bi[:, three]][:, :, None] * sd[bi[:, two]][:, None, :],
                           "odom_cross": sd[oi[:, :3]][:, :, None] * sd[oi[:, 3:]][:, None, :],
                           "bearing_var": (np.abs(Jb) * sd[bi]).sum(axis=1) ** 2,
                           "odom_cov": so[:, :, None] * so[:, None, :]}
        del star_full
        self.full = None            # the cached references keep the edges' entries only, no N x N matrix
        self.e_lu, self.e_chol = ({"blocks": e} for e in (self.refined.e_lu, self.refined.e_chol))
        for X, e in ((d.lu, self.e_lu), (d.chol, self.e_chol)):
            ent = edge_entries(P, d.full(X), pose, lm)[0]
            for group in self.KEYS:
                errs = self.edge_errors(group, ent)
                e[group] = float(errs.max()) if len(errs) else 0.0
        self.e_ref = {g: max(self.e_lu[g], self.e_chol[g]) for g in self.e_lu}

    def edge_errors(self, group, out):
        """[Mb + Mo] (bearings, then odometry): per edge, the largest scaled error of its cross block
        (group "cross") or its projected covariance ("projected") in the result dict out, against Sigma*.
        Where the scale is zero (only the fixed pose's dofs are involved) the output must be exactly zero."""
        each = []
        for k in self.KEYS[group]:
            o, ref, scale = out[k], self.star[k], self.star_scale[k]
            zero = scale == 0.0
            assert np.all(o[zero] == 0.0), "an entry of the fixed pose alone is not exactly zero"
            err = np.zeros(o.shape)
            err[~zero] = (np.abs(o - ref)[~zero] / scale[~zero]).astype(np.float64)
            each.append(err.reshape(len(o), -1).max(axis=1) if len(o) else np.zeros(0))
        return np.concatenate(each)


def check_refined(ref, out, label=""):
    """The refined criterion on one result dict: e <= MARGIN e_ref for the blocks, the cross blocks and
    the projected covariances, each against its own e_ref. Prints e, e_ref (LU / Cholesky) and the
    ratio of each group before asserting; returns the per-node and per-edge errors."""
    errs = {"blocks": ref.refined.errors(out["pose_cov"], out["landmark_cov"]),
            "cross": ref.edge_errors("cross", out), "projected": ref.edge_errors("projected", out)}
    worst = {g: float(v.max()) if len(v) else 0.0 for g, v in errs.items()}
    for g, e in worst.items():
        print(f"  refined {label} {g}: e {e:.3g} e_ref {ref.e_ref[g]:.3g} (lu {ref.e_lu[g]:.3g} / chol {ref.e_chol[g]:.3g}) "
              f"ratio {ratio(e, ref.e_ref[g]):.3g}")
    for g, e in worst.items():
        assert e <= MARGIN * ref.e_ref[g], (label, g, e, ref.e_ref[g], ratio(e, ref.e_ref[g]))
    return errs


def check_reference(ref, out, tol_cap):
    """The reference bounds on one result dict: tol <= tol_cap first, the diagonal blocks and the cross
    blocks within tol, the projected covariances within 2 tol. Returns the three errors."""
    assert ref.tol <= tol_cap
    eb = ref.error(out["pose_cov"], out["landmark_cov"])
    ec = ref.cross_error(out["bearing_cross"], out["odom_cross"])
    ep = ref.projected_error(out["bearing_var"], out["odom_cov"])
    print(f"  n {ref.n} kappa_1 {ref.kappa:.3g} tol {ref.tol:.3g}: blocks {eb:.3g} cross {ec:.3g} projected {ep:.3g}")
    assert eb <= ref.tol
    assert ec <= ref.tol
    assert ep <= 2 * ref.tol
    return eb, ec, ep


def check_structure(P, out):
    """The exact rules of bos_edge_covariances (include/bos.h) on one result dict."""
    bc, oc, bv, ov, pc = out["bearing_cross"], out["odom_cross"], out["bearing_var"], out["odom_cov"], out["pose_cov"]
    fx = P.fixed
    assert np.all(pc[fx] == 0.0)
    assert np.all(bc[P.b_pose == fx] == 0.0)
    assert np.all(oc[(P.o_src == fx) | (P.o_dst == fx)] == 0.0)
    assert np.array_equal(ov, ov.transpose(0, 2, 1))            # mirrored lower triangle
    assert np.all(bv > 0.0)
    loops = np.nonzero(P.o_src == P.o_dst)[0]
    for e in loops:                                             # a self-loop's cross block is S_aa
        assert np.array_equal(oc[e], pc[P.o_src[e]])
    # duplicates: identical bits in one orientation, the transposed cross block in the other
    seen = {}
    for e, (p, l) in enumerate(zip(P.b_pose, P.b_lm)):
        f = seen.setdefault((int(p), int(l)), e)
        if f != e:
            assert np.array_equal(bc[e], bc[f]) and bv[e] == bv[f]
    seen = {}
    for e, (a, b) in enumerate(zip(P.o_src, P.o_dst)):
        f = seen.setdefault((int(a), int(b)), e)
        if f != e:
            assert np.array_equal(oc[e], oc[f]) and np.array_equal(ov[e], ov[f])
        g = seen.get((int(b), int(a)))
        if g is not None and g != e:
            assert np.array_equal(oc[e], oc[g].T)


def check_information_bound(P, out):
    """A bound that needs no reference: H >= J^T Omega J for every edge (the build keeps the unscaled
    J^T Omega J under the robust kernel) plus the damping, so omega bearing_var < 1 for every bearing and
    the largest eigenvalue of Omega^1/2 odom_cov Omega^1/2 is < 1 for every odometry edge that is not
    a self-loop."""
    w = np.ones(len(P.b_z)) if P.b_omega is None else P.b_omega
    assert np.all(w * out["bearing_var"] < 1.0), float((w * out["bearing_var"]).max())
    keep = P.o_src != P.o_dst
    if keep.any():
        L = np.linalg.cholesky(P.o_omega[keep])                 # Omega = L L^T: eig(L^T C L) = eig(Omega^1/2 C Omega^1/2)
        M = np.einsum("mji,mjk,mkl->mil", L, out["odom_cov"][keep], L)
        top = np.linalg.eigvalsh(0.5 * (M + M.transpose(0, 2, 1)))[:, -1]
        assert np.all(top < 1.0), float(top.max())
