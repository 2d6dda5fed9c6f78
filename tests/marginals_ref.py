"""Reference and error measure shared by the marginal-covariance tests (host and GPU).

Reference: Sigma_ref = inv(H), H the symmetrised H_nf without the fixed pose, dense fp64.
Error: e = max |Sigma_out[i, j] - Sigma_ref[i, j]| / sqrt(Sigma_ref[i, i] Sigma_ref[j, j]) over every
entry of every returned block (a correlation-scaled absolute error).
Bound: tol = n eps kappa_1(H_s), H_s = D^-1/2 H D^-1/2 with D = diag H: the forward-error bound of a
Cholesky-based inverse in its Jacobi-scaled form; kappa_1 = |H_s|_1 |H_s^-1|_1 comes from Sigma_ref
itself (H_s^-1 = D^1/2 Sigma_ref D^1/2). Every accuracy test asserts tol <= 1e-6 first, so the bound
stays sharp."""
import numpy as np

EPS = 2.22e-16
TOL_CAP = 1e-6


class Reference:
    """Sigma_ref and tol of the lower triangle Hl (scipy sparse, reference dof numbering, N x N) of a
    problem P (bos.Problem)."""

    def __init__(self, P, Hl):
        Hl = Hl.tocsr()
        keep = np.ones(P.N, dtype=bool)
        keep[3 * P.fixed:3 * P.fixed + 3] = False
        self.idx = np.nonzero(keep)[0]
        Hd = Hl.toarray()
        H = Hd + np.tril(Hd, -1).T
        H = H[np.ix_(self.idx, self.idx)]
        n = H.shape[0]
        S = np.linalg.inv(H)
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
