"""Reference and error measure shared by the marginal-covariance tests (host and GPU).

Reference: Sigma_ref = inv(H), H the symmetrised H_nf without the fixed pose, dense fp64.
Error: e = max |Sigma_out[i, j] - Sigma_ref[i, j]| / sqrt(Sigma_ref[i, i] Sigma_ref[j, j]) over every
entry of every returned block (a correlation-scaled absolute error).
Bound: tol = n eps kappa_1(H_s), H_s = D^-1/2 H D^-1/2 with D = diag H: the forward-error bound of a
Cholesky-based inverse in its Jacobi-scaled form; kappa_1 = |H_s|_1 |H_s^-1|_1 comes from Sigma_ref
itself (H_s^-1 = D^1/2 Sigma_ref D^1/2). Every accuracy test asserts tol <= 1e-6 first, so the bound
stays sharp.

The refined criterion (RefinedReference, and RefinedEdgeReference in edge_cov_ref.py) closes the five
orders of magnitude between tol and what a correct fp64 recursion gives. Its reference is
Sigma* = X0 + X0 R, X0 = numpy.linalg.inv(H) and R = I - H X0 evaluated in np.longdouble (one Newton
step: the error of X0, about 1e-12 in the measure above, is squared away down to the rounding of R,
which is 2^11 times finer than anything computed in fp64). The error measure is the one above with
Sigma* in Sigma_ref's place. Its bound is measured, never derived from the result: e_ref is the larger
error, in the same measure over the same returned entries, of two plain fp64 inverses of that very H
(LU: numpy.linalg.inv; Cholesky: cho_factor + cho_solve(I)), and a result passes when
e <= MARGIN e_ref = 8 e_ref. The margin is the solver route tests' backward-error margin; it covers
another elimination order and the MFMA / FMA summation order. A single entry off by 1e-9 of its scale
fails it on every system with tol >= 1e-8 and passes the old bound (tests/test_selinv_criterion_host.py)."""
import numpy as np

EPS = 2.22e-16
TOL_CAP = 1e-6
MARGIN = 8.0


def dense_system(P, Hl):
    """(idx, H): the free dofs (reference numbering) and the dense symmetrised H_nf over them."""
    keep = np.ones(P.N, dtype=bool)
    keep[3 * P.fixed:3 * P.fixed + 3] = False
    idx = np.nonzero(keep)[0]
    Hd = Hl.tocsr().toarray()
    H = Hd + np.tril(Hd, -1).T
    return idx, np.ascontiguousarray(H[np.ix_(idx, idx)])


class DenseInverses:
    """The three dense inverses of one H the refined criterion needs: lu = numpy.linalg.inv(H), chol =
    cho_solve(cho_factor(H), I), both plain fp64, and star = lu + lu R with R = I - H lu in
    np.longdouble, H's rows taken sparse (nnz n long multiplications). residual = max |R|."""

    def __init__(self, P, Hl):
        import scipy.linalg as sla
        self.N = P.N
        self.idx, self.H = dense_system(P, Hl)
        H, n = self.H, len(self.idx)
        self.lu = np.linalg.inv(H)
        self.chol = sla.cho_solve(sla.cho_factor(H, lower=True), np.eye(n))
        Xl = self.lu.astype(np.longdouble)
        R = np.empty((n, n), dtype=np.longdouble)
        for i in range(n):
            c = np.nonzero(H[i])[0]
            R[i] = -(H[i, c].astype(np.longdouble)[:, None] * Xl[c]).sum(axis=0)
            R[i, i] += 1
        self.residual = float(np.abs(R).max())
        self.star = Xl + (self.lu @ R.astype(np.float64)).astype(np.longdouble)

    def full(self, X):
        """X padded with zeros for the fixed pose: N x N in the reference dof numbering."""
        out = np.zeros((self.N, self.N), dtype=X.dtype)
        out[np.ix_(self.idx, self.idx)] = X
        return out


def node_blocks(P, full):
    """(pose [NP, 3, 3], lm [NL, 2, 2]): the nodes' diagonal blocks of a padded N x N matrix."""
    NP, NL = P.NP, P.NL
    pose = np.stack([full[3 * u:3 * u + 3, 3 * u:3 * u + 3] for u in range(NP)])
    lm = (np.stack([full[3 * NP + 2 * l:3 * NP + 2 * l + 2, 3 * NP + 2 * l:3 * NP + 2 * l + 2] for l in range(NL)])
          if NL else np.zeros((0, 2, 2), dtype=full.dtype))
    return pose, lm


def ratio(e, e_ref):
    return e / e_ref if e_ref > 0.0 else (0.0 if e == 0.0 else float("inf"))


class RefinedBlocks:
    """The diagonal blocks' part of the refined criterion: Sigma*'s blocks, its standard deviations and
    e_ref of the two fp64 inverses (lu, chol), from a DenseInverses d."""

    def __init__(self, P, d, star_full=None):
        star_full = d.full(d.star) if star_full is None else star_full
        self.fixed = P.fixed
        self.pose, self.lm = node_blocks(P, star_full)
        self.sd = np.sqrt(np.diag(star_full))                       # [N], zero on the fixed pose
        self.e_lu = float(self.errors(*node_blocks(P, d.full(d.lu))).max())
        self.e_chol = float(self.errors(*node_blocks(P, d.full(d.chol))).max())
        self.e_ref = max(self.e_lu, self.e_chol)

    def errors(self, pose_cov, lm_cov):
        """[NP + NL]: per node, max |out - Sigma*| / (sd_i sd_j) over its block (0 for the fixed pose,
        whose block is compared with zero by check_blocks)."""
        NP = len(self.pose)
        sp = self.sd[:3 * NP].reshape(-1, 3).copy()
        sp[self.fixed] = 1.0
        sl = self.sd[3 * NP:].reshape(-1, 2)
        ep = (np.abs(pose_cov - self.pose) / (sp[:, :, None] * sp[:, None, :])).max(axis=(1, 2))
        ep[self.fixed] = 0.0
        el = (np.abs(lm_cov - self.lm) / (sl[:, :, None] * sl[:, None, :])).max(axis=(1, 2)) if len(self.lm) else np.zeros(0)
        return np.concatenate([ep, el]).astype(np.float64)


class Reference:
    """Sigma_ref and tol of the lower triangle Hl (scipy sparse, reference dof numbering, N x N) of a
    problem P (bos.Problem). dense: a DenseInverses of the same P and Hl, whose lu is then Sigma_ref."""

    def __init__(self, P, Hl, dense=None):
        if dense is None:
            self.idx, H = dense_system(P, Hl)
            S = np.linalg.inv(H)
        else:
            self.idx, H, S = dense.idx, dense.H, dense.lu
        n = H.shape[0]
        d = np.sqrt(np.diag(H))
        Hs = H / np.outer(d, d)
        Hsi = S * np.outer(d, d)
        self.kappa = float(np.abs(Hs).sum(axis=0).max() * np.abs(Hsi).sum(axis=0).max())
        self.tol = n * EPS * self.kappa
        self.n = n
        full = np.zeros((P.N, P.N))
        full[np.ix_(self.idx, self.idx)] = S
        NP, NL = P.NP, P.NL
        self.pose = np.stack([full[3 * u:3 * u + 3, 3 * u:3 * u + 3] for u in range(NP)])
        self.lm = (np.stack([full[3 * NP + 2 * l:3 * NP + 2 * l + 2, 3 * NP + 2 * l:3 * NP + 2 * l + 2] for l in range(NL)])
                   if NL else np.zeros((0, 2, 2)))
        self.fixed = P.fixed

    def error(self, pose_cov, lm_cov):
        """The scaled error of the returned blocks (the fixed pose's block is not compared)."""
        e = 0.0
        for out, ref in ((pose_cov, self.pose), (lm_cov, self.lm)):
            for u in range(len(ref)):
                if out is pose_cov and u == self.fixed:
                    continue
                s = np.sqrt(np.diag(ref[u]))
                e = max(e, float((np.abs(out[u] - ref[u]) / np.outer(s, s)).max()))
        return e


class RefinedReference(Reference):
    """Reference (the old bound's Sigma_ref and tol, unchanged) plus the refined criterion for the
    diagonal blocks: .refined is a RefinedBlocks, .residual the Newton step's max |I - H X0|."""

    def __init__(self, P, Hl):
        d = DenseInverses(P, Hl)
        super().__init__(P, Hl, dense=d)
        self.residual = d.residual
        self.refined = RefinedBlocks(P, d)

    def check_refined(self, pose_cov, lm_cov, label=""):
        """e <= MARGIN e_ref for the blocks; prints e, e_ref (LU / Cholesky) and the ratio, returns the
        per-node errors."""
        return check_refined_blocks(self.refined, pose_cov, lm_cov, label)


def check_refined_blocks(rb, pose_cov, lm_cov, label=""):
    errs = rb.errors(pose_cov, lm_cov)
    e = float(errs.max())
    print(f"  refined {label} blocks: e {e:.3g} e_ref {rb.e_ref:.3g} (lu {rb.e_lu:.3g} / chol {rb.e_chol:.3g}) "
          f"ratio {ratio(e, rb.e_ref):.3g}")
    assert e <= MARGIN * rb.e_ref, (label, e, rb.e_ref, ratio(e, rb.e_ref))
    return errs


def sparse_tol(P, Hl):
    """tol = n eps kappa_1(H_s) without a dense inverse (systems too large for one): |H_s|_1 exactly,
    |H_s^-1|_1 by Higham's 1-norm estimator over a sparse LU solve. The estimate never exceeds the
    norm, so this bound is never wider than the dense one."""
    import scipy.sparse as sp
    import scipy.sparse.linalg as spla
    keep = np.ones(P.N, dtype=bool)
    keep[3 * P.fixed:3 * P.fixed + 3] = False
    idx = np.nonzero(keep)[0]
    Hl = Hl.tocsr()
    H = (Hl + sp.tril(Hl, -1).T).tocsr()[idx][:, idx]
    d = 1.0 / np.sqrt(H.diagonal())
    Hs = (sp.diags(d) @ H @ sp.diags(d)).tocsc()
    lu = spla.splu(Hs)
    n = Hs.shape[0]
    inv = spla.LinearOperator((n, n), matvec=lu.solve, rmatvec=lu.solve, dtype=np.float64)   # H_s symmetric
    kappa = float(abs(Hs).sum(axis=0).max() * spla.onenormest(inv))
    return n * EPS * kappa, kappa


def scaled_diff(pa, la, pb, lb, ref):
    """max |a - b| / sqrt(Sigma_ref[i, i] Sigma_ref[j, j]) between two sets of blocks."""
    e = 0.0
    for a, b, r, skip in ((pa, pb, ref.pose, ref.fixed), (la, lb, ref.lm, -1)):
        for u in range(len(r)):
            if u == skip:
                continue
            s = np.sqrt(np.diag(r[u]))
            e = max(e, float((np.abs(a[u] - b[u]) / np.outer(s, s)).max()))
    return e


def check_blocks(P, pose_cov, lm_cov):
    """Structure every plan must give: the fixed pose's block exactly zero, every block symmetric bit
    for bit with positive diagonal entries."""
    assert np.all(pose_cov[P.fixed] == 0.0)
    assert np.array_equal(pose_cov, pose_cov.transpose(0, 2, 1))
    assert np.array_equal(lm_cov, lm_cov.transpose(0, 2, 1))
    free = np.arange(P.NP) != P.fixed
    assert np.all(np.diagonal(pose_cov[free], axis1=1, axis2=2) > 0.0)
    assert np.all(np.diagonal(lm_cov, axis1=1, axis2=2) > 0.0)
