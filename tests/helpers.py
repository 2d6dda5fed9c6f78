"""Shared helpers for the parity tests: convert between the product's problem (bos.Problem)
and the oracle's (oracle.Problem), and bring both H's into one comparable form."""
import contextlib
import itertools

import numpy as np
import scipy.sparse as sp

import bos
import oracle as O


def to_oracle(P: "bos.Problem") -> "O.Problem":
    """Same arrays, same initial state: parity tests start the oracle and the HIP path from
    identical inputs (the product's own triangulation is checked separately)."""
    return O.Problem(pose_ids=P.pose_ids, lm_ids=P.lm_ids, pose_xyt=P.pose_xyt.copy(), lm_xy=P.lm_xy.copy(),
                     b_pose=P.b_pose.copy(), b_lm=P.b_lm.copy(), b_z=P.b_z.copy(),
                     b_omega=None if P.b_omega is None else P.b_omega.copy(), o_src=P.o_src.copy(),
                     o_dst=P.o_dst.copy(), o_z=P.o_z.copy(), o_omega=P.o_omega.copy(), fixed=P.fixed)


def oracle_lower_nf(Q: "O.Problem", lin) -> sp.csr_matrix:
    """Lower triangle of H with the fixed pose's rows/cols removed (kept in N numbering)."""
    H = O.assemble_H(Q, lin).tocoo()
    keep = np.ones(Q.N, dtype=bool)
    keep[3 * Q.fixed:3 * Q.fixed + 3] = False
    m = (H.row >= H.col) & keep[H.row] & keep[H.col]
    return sp.coo_matrix((H.data[m], (H.row[m], H.col[m])), shape=H.shape).tocsr()


def gpu_lower(rows, cols, vals, N) -> sp.csr_matrix:
    return sp.coo_matrix((vals, (rows.astype(np.int64), cols.astype(np.int64))), shape=(N, N)).tocsr()


def rel_err(a: sp.spmatrix, b: sp.spmatrix) -> float:
    d = (a - b).tocoo()
    scale = max(abs(a).max(), abs(b).max(), 1e-300)
    return (np.abs(d.data).max() if d.nnz else 0.0) / scale


def state_rel_err(pa, la, pb, lb, floor=1e-9):
    """max |a - b| / max(|b|, floor) over poses (x, y, wrapped theta) and landmarks."""
    dp = pa - pb
    dp[:, 2] = (dp[:, 2] + np.pi) % (2 * np.pi) - np.pi
    e1 = np.abs(dp) / np.maximum(np.abs(pb), floor)
    e2 = np.abs(la - lb) / np.maximum(np.abs(lb), floor) if len(lb) else np.zeros(1)
    return max(e1.max(), e2.max())


def close_state(pa, la, pb, lb, rtol=1e-6, atol=1e-9):
    dp = pa - pb
    dp[:, 2] = (dp[:, 2] + np.pi) % (2 * np.pi) - np.pi
    ok_p = np.all(np.abs(dp) <= rtol * np.abs(pb) + atol)
    ok_l = np.all(np.abs(la - lb) <= rtol * np.abs(lb) + atol)
    return ok_p and ok_l, float(np.abs(dp).max()), float(np.abs(la - lb).max() if len(lb) else 0.0)


def knife_edge_bearings(P, tol=1e-9):
    """Bearings whose error (the oracle's literal evaluation, at P's state) lies on the +-pi wrap:
    their sign is decided by the last ulp of atan2 and g (the reference dataset's single-observation
    landmarks after triangulation)."""
    with O.literal():
        e = O.bearing_errors(P)
    return np.nonzero(np.abs(e) >= np.pi - tol)[0], e


def wrap_signs_from_gpu(P, b_gpu, kt=1.0):
    """The sign the GPU path gave each knife-edge bearing's error, read off its exported b (fp64,
    P's state): flipping bearing k's error changes b by -2 J_k^T w e_k (robust-scaled e_k) on its
    pose's and landmark's dofs; the combination of flips that reproduces the GPU's b (to 1e-9 of
    max |b|) gives the signs. None when P has no such bearing. The oracle then evaluates every
    bearing literally (Eigen's product sums, libm atan2: no code shared with the product) and only
    takes these signs from the GPU (bos_oracle.cpp knife_edge)."""
    ks, e = knife_edge_bearings(P)
    if len(ks) == 0:
        return None
    # The only bearings whose sign may be taken from the GPU are the sole observations of their
    # landmark (triangulated onto their own ray); on the reference dataset exactly
    # the three on landmarks 69, 112 and 114 (the set cannot grow silently). Their sign
    # is parity-unpinned.
    counts = np.bincount(P.b_lm, minlength=P.NL)
    assert np.all(counts[P.b_lm[ks]] == 1), [int(k) for k in ks if counts[P.b_lm[k]] != 1]
    if getattr(P, "lm_ids", None) is not None and P.NP == 301 and P.NL == 141:
        assert sorted(int(P.lm_ids[P.b_lm[k]]) for k in ks) == [69, 112, 114], ks
    Q = to_oracle(P)
    with O.literal():
        lin = O.linearize(Q, kernel_threshold=kt)
        contrib = []
        for k in ks:
            ek, J = O.bearing_error_and_jacobian(P.pose_xyt[P.b_pose[k]], P.lm_xy[P.b_lm[k]], P.b_z[k])
            w = 1.0 if P.b_omega is None else float(P.b_omega[k])
            rho = ek * w * ek
            es = ek * np.sqrt(kt / rho) if rho > kt else ek
            d = np.zeros(P.N)
            d[3 * P.b_pose[k]:3 * P.b_pose[k] + 3] = J[:3] * w * es
            d[3 * P.NP + 2 * P.b_lm[k]:3 * P.NP + 2 * P.b_lm[k] + 2] = J[3:] * w * es
            contrib.append(d)
    keep = np.ones(P.N, dtype=bool)
    keep[3 * P.fixed:3 * P.fixed + 3] = False
    best, best_flip = None, None
    for flips in itertools.product((False, True), repeat=len(ks)):
        alt = lin.b - sum(2 * c for c, f in zip(contrib, flips) if f)
        err = np.abs(b_gpu - alt)[keep].max()
        if best is None or err < best:
            best, best_flip = err, flips
    assert best <= 1e-9 * np.abs(lin.b[keep]).max(), f"no sign combination of the knife-edge bearings reproduces b ({best})"
    signs = np.zeros(len(P.b_z), dtype=np.int8)
    for k, f in zip(ks, best_flip):
        signs[k] = -int(np.sign(e[k])) if f else int(np.sign(e[k]))
    return signs


@contextlib.contextmanager
def literal_oracle(P, b_gpu=None, kt=1.0):
    """The oracle in its literal form for the block, with the knife-edge bearings' signs taken from
    the GPU path's b at P's initial state (b_gpu, or one fp64 GPU linearization made here)."""
    if b_gpu is None and len(knife_edge_bearings(P)[0]):
        S = bos.Solver(P, kernel_threshold=kt)
        S.linearize()
        b_gpu = S.export_system()[3]
        S.close()
    signs = None if b_gpu is None else wrap_signs_from_gpu(P, b_gpu, kt)
    with O.literal(wrap_signs=signs):
        yield signs


def lin_parity(P, precision=bos.BOS_FP64, kt=1.0, damping=0.01, tol=1e-12, p999=None, btol=None, **solver_kw):
    """H, b, chi^2 of one GPU J+H build against the oracle's literal evaluation (knife-edge
    bearings' signs from the GPU's fp64 b, literal_oracle)."""
    Q = to_oracle(P)
    S = bos.Solver(P, precision=precision, kernel_threshold=kt, damping=damping, **solver_kw)
    st = S.linearize()
    rows, cols, vals, b = S.export_system()
    b64 = b
    if precision != bos.BOS_FP64 and len(knife_edge_bearings(P)[0]):
        S64 = bos.Solver(P, kernel_threshold=kt, damping=damping, **solver_kw)
        S64.linearize()
        b64 = S64.export_system()[3]
        S64.close()
    with literal_oracle(P, b64, kt):
        lin = O.linearize(Q, kernel_threshold=kt, damping=damping, precision=32 if precision == bos.BOS_FP32 else 64)
    Hg = gpu_lower(rows, cols, vals, P.N)
    Ho = oracle_lower_nf(Q, lin)
    eh = rel_err(Hg, Ho)
    # b of the fixed pose is discarded by the reference (solver.cpp:73) and not produced here
    keep = np.ones(P.N, dtype=bool)
    keep[3 * P.fixed:3 * P.fixed + 3] = False
    assert np.all(b[~keep] == 0.0)
    eb = np.abs(b - lin.b)[keep].max() / max(np.abs(lin.b[keep]).max(), 1e-300)
    assert eh <= tol, f"H rel err {eh}"
    assert eb <= (10 * tol if btol is None else btol), f"b rel err {eb}"
    if p999 is not None:
        # scale-invariant per-entry error |dH_ij| / sqrt(H_ii H_jj) (bounded by 1 for SPD H)
        d = (Hg - Ho).tocoo()
        dg = np.abs(Ho.diagonal())
        per = np.abs(d.data) / np.sqrt(np.maximum(dg[d.row] * dg[d.col], 1e-300))
        assert np.quantile(per, 0.999) <= p999, np.quantile(per, 0.999)
    if precision == bos.BOS_FP64:
        assert abs(st["chi2"] - lin.chi2) <= 1e-9 * max(lin.chi2, 1.0)
        assert st["n_robust"] == lin.n_robust
    else:
        assert abs(st["chi2"] - lin.chi2) <= 1e-3 * max(lin.chi2, 1.0)
    S.close()
    return eh, eb


class SolveReference:
    """H_nf x = b of one exported system, solved to (nearly) working precision of np.longdouble.
    Vectors are in the reduced numbering: the reference dofs `idx` (the fixed pose's three removed)."""

    def __init__(self, H, b, idx, x):
        self.H, self.b, self.idx, self.x = H, b, idx, x
        self._Hl, self._bl = H.astype(np.longdouble), b.astype(np.longdouble)
        self._normH = float(np.abs(H).sum(axis=1).max())
        self._unrefined = None

    def fwd(self, x):
        """Forward error ||x - x*||_inf / ||x*||_inf."""
        return float(np.abs(np.asarray(x, dtype=np.longdouble) - self.x).max() / np.abs(self.x).max())

    def eta(self, x):
        """Normwise backward error ||b - H x||_inf / (||H||_inf ||x||_inf + ||b||_inf), residual in longdouble."""
        xl = np.asarray(x, dtype=np.longdouble)
        r = self._bl - self._Hl @ xl
        return float(np.abs(r).max() / (self._normH * float(np.abs(xl).max()) + np.abs(self.b).max()))

    def unrefined(self):
        """(fwd, eta) of the two plain fp64 solvers the criterion measures its bound from, on this very
        system: dense LAPACK Cholesky and SciPy SuperLU, neither refined."""
        if self._unrefined is None:
            import scipy.linalg as sla
            import scipy.sparse.linalg as spla
            xc = sla.cho_solve(sla.cho_factor(self.H, lower=True), self.b)
            xs = spla.splu(sp.csc_matrix(self.H)).solve(self.b)
            self._unrefined = {"chol": (self.fwd(xc), self.eta(xc)), "splu": (self.fwd(xs), self.eta(xs))}
        return self._unrefined

    def check(self, x, label=""):
        """The solve criterion: fwd(x) <= 4 max(fwd_chol, fwd_splu) and eta(x) <= 8 max(eta_chol, eta_splu).
        The bound comes from the two reference solvers on this system, never from x. Returns
        (fwd, eta, fwd_bound / 4, eta_bound / 8, ok) and prints the four numbers."""
        u = self.unrefined()
        f_ref = max(u["chol"][0], u["splu"][0])
        e_ref = max(u["chol"][1], u["splu"][1])
        f, e = self.fwd(x), self.eta(x)
        print(f"solve {label}: fwd {f:.3e} (ref max {f_ref:.3e}, ratio {f / f_ref:.3g}) "
              f"eta {e:.3e} (ref max {e_ref:.3e}, ratio {e / e_ref:.3g})")
        return f, e, f_ref, e_ref, bool(f <= 4 * f_ref and e <= 8 * e_ref)


def solve_reference(rows, cols, vals, b, fixed, max_iter=60):
    """x* of the exported system (bos_export_system: lower triangle of H_nf in reference dof numbering,
    full b) with the fixed pose's dofs removed: dense LAPACK Cholesky, then iterative refinement with
    the residual and the accumulated solution in np.longdouble until the correction is below 1e-18 of
    ||x||_inf. Where cond(H) eps_longdouble lies above 1e-18 the corrections settle at that level
    instead; the refinement then stops once a correction is no smaller than half the one before (x* is
    still ~2^11 times finer than any fp64 solve of the system). Returns a SolveReference."""
    import scipy.linalg as sla
    N = len(b)
    r64, c64 = np.asarray(rows, dtype=np.int64), np.asarray(cols, dtype=np.int64)
    H = np.zeros((N, N))
    np.add.at(H, (r64, c64), vals)
    off = r64 != c64
    np.add.at(H, (c64[off], r64[off]), np.asarray(vals)[off])
    keep = np.ones(N, dtype=bool)
    keep[3 * fixed:3 * fixed + 3] = False
    idx = np.nonzero(keep)[0]
    H = np.ascontiguousarray(H[np.ix_(idx, idx)])
    bn = np.asarray(b, dtype=np.float64)[idx]
    cf = sla.cho_factor(H, lower=True)
    Hl, bl = H.astype(np.longdouble), bn.astype(np.longdouble)
    x = sla.cho_solve(cf, bn).astype(np.longdouble)
    last = np.inf
    for _ in range(max_iter):
        r = bl - Hl @ x
        d = sla.cho_solve(cf, r.astype(np.float64)).astype(np.longdouble)
        x = x + d
        rel = float(np.abs(d).max() / np.abs(x).max())
        if rel < 1e-18 or rel > 0.5 * last:
            break
        last = rel
    return SolveReference(H, bn, idx, x)


def joined_world(A, B, seed=9):
    """Two worlds made one problem: B's poses and landmarks follow A's, and one odometry edge from A's
    last pose to B's first (measured from the current estimates plus noise, the information of A's
    first edge) ties B to A's fixed pose. The pose graph's only link between the two is that edge, so
    a nested dissection cuts there and the two halves become sibling subtrees of different front sizes."""
    rng = np.random.default_rng(seed)
    s, d = A.NP - 1, A.NP
    z = O.predict_odometry(A.pose_xyt[s], B.pose_xyt[0]) + rng.normal(0, 0.02, 3)
    return bos.Problem(np.concatenate([A.pose_xyt, B.pose_xyt]), np.concatenate([A.lm_xy, B.lm_xy]),
                       np.concatenate([A.b_pose, B.b_pose + A.NP]), np.concatenate([A.b_lm, B.b_lm + A.NL]),
                       np.concatenate([A.b_z, B.b_z]), np.concatenate([A.o_src, B.o_src + A.NP, [s]]),
                       np.concatenate([A.o_dst, B.o_dst + A.NP, [d]]), np.concatenate([A.o_z, B.o_z, z[None]]),
                       np.concatenate([A.o_omega, B.o_omega, A.o_omega[:1]]), A.fixed)


# The worlds of the solver route tests (tests/test_gpu_solver_routes.py, and the criterion's own CPU
# test in tests/test_host.py): name -> (world, solver, schur_leaf). A world is the arguments of
# bos.synthetic(..., seed=5), or two of them for joined_world. All with damping 0.01 (at damping 0 the
# (65, 257, 8) world's H is singular: it has unobserved landmarks). DESIGN.md §5 has the routes each takes.
SOLVER_WORLDS = {
    "12_sn": ((12, 6, 3), bos.BOS_SOLVER_SUPERNODAL, 0),
    "12_schur": ((12, 6, 3), bos.BOS_SOLVER_SCHUR, 0),
    "40_schur_leaf40": ((40, 40, 4), bos.BOS_SOLVER_SCHUR, 40),
    "65_schur_leaf80": ((65, 257, 8), bos.BOS_SOLVER_SCHUR, 80),
    "200_schur": ((200, 300, 8), bos.BOS_SOLVER_SCHUR, 0),
    "300_sn": ((300, 600, 10), bos.BOS_SOLVER_SUPERNODAL, 0),
    "100_schur_leaf30": ((100, 100, 4), bos.BOS_SOLVER_SCHUR, 30),
    "150_sn": ((150, 300, 20), bos.BOS_SOLVER_SUPERNODAL, 0),
    "joined_schur_leaf80": (((45, 260, 12), (40, 40, 4)), bos.BOS_SOLVER_SCHUR, 80),
}
SOLVER_DAMPING = 0.01
_solver_world_cache = {}


def solver_world(name):
    """(problem, solver, schur_leaf) of a SOLVER_WORLDS entry; the problem is built once."""
    if name not in _solver_world_cache:
        w, solver, leaf = SOLVER_WORLDS[name]
        if isinstance(w[0], tuple):
            P = joined_world(bos.synthetic(*w[0], seed=5), bos.synthetic(*w[1], seed=5))
        else:
            P = bos.synthetic(*w, seed=5)
        _solver_world_cache[name] = (P, solver, leaf)
    return _solver_world_cache[name]


# ---------------------------------------------------------------- 50-digit references (mpmath)
EPS = 2.220446049250313e-16
MP_DIGITS = 50


def _mp():
    import mpmath
    mpmath.mp.dps = MP_DIGITS
    return mpmath


def landmark_observations(P):
    """Per landmark, its bearings' indices in file order (what bos_create's CSR build must produce)."""
    order = np.argsort(P.b_lm, kind="stable")
    ptr = np.concatenate([[0], np.cumsum(np.bincount(P.b_lm, minlength=P.NL))])
    return [order[ptr[l]:ptr[l + 1]] for l in range(P.NL)]


def mp_triangulate(P, pose_xyt):
    """The triangulation of every landmark from the exact double inputs, at 50 digits: the rows
    [sin(th + z), -cos(th + z)] and right-hand sides sin(th + z) px - cos(th + z) py of
    slam/triangulation.cpp, then per landmark a dict with
      M, n0, n1          the number of rows and the two squared column norms,
      basic              the two basic solutions ((c0.r / n0, 0), (0, c1.r / n1)), None where the column is 0,
      xy, kappa          the least-squares solution (normal equations) and kappa_2 of the rows from the
                         2 x 2 Gram matrix; None for M < 2 or a Gram determinant of 0,
      pmax               max |p_xy| over the landmark's poses.
    All numbers are mpmath values."""
    mp = _mp()
    sc = {}
    out = []
    for ks in landmark_observations(P):
        n0 = n1 = g = b0 = b1 = mp.mpf(0)
        pmax = 0.0
        for k in ks:
            p = pose_xyt[P.b_pose[k]]
            key = (float(p[2]), float(P.b_z[k]))
            if key not in sc:
                ang = mp.mpf(key[0]) + mp.mpf(key[1])
                sc[key] = (mp.sin(ang), mp.cos(ang))
            s, c = sc[key]
            a0, a1 = s, -c
            r = s * mp.mpf(float(p[0])) - c * mp.mpf(float(p[1]))
            n0, n1, g, b0, b1 = n0 + a0 * a0, n1 + a1 * a1, g + a0 * a1, b0 + a0 * r, b1 + a1 * r
            pmax = max(pmax, abs(float(p[0])), abs(float(p[1])))
        d = dict(M=len(ks), n0=n0, n1=n1, pmax=pmax, xy=None, kappa=None,
                 basic=((b0 / n0, mp.mpf(0)) if n0 > 0 else None, (mp.mpf(0), b1 / n1) if n1 > 0 else None))
        det = n0 * n1 - g * g
        if len(ks) >= 2 and det > 0:
            d["xy"] = ((n1 * b0 - g * b1) / det, (n0 * b1 - g * b0) / det)
            lmax = (n0 + n1 + mp.sqrt((n0 - n1) ** 2 + 4 * g * g)) / 2
            d["kappa"] = mp.sqrt(lmax / (det / lmax))
        out.append(d)
    return out


def mp_boxplus(pose0, dpose):
    """The left-multiplicative box-plus of every pose at 50 digits from the exact doubles:
    x' = cos(dth) x - sin(dth) y + dx, y' = sin(dth) x + cos(dth) y + dy, th' = th + dth (not wrapped).
    Returns a list of (x', y', th') mpmath triples."""
    mp = _mp()
    out = []
    for (x, y, th), (dx, dy, dth) in zip(pose0, dpose):
        x, y, th, dx, dy, dth = (mp.mpf(float(v)) for v in (x, y, th, dx, dy, dth))
        c, s = mp.cos(dth), mp.sin(dth)
        out.append((c * x - s * y + dx, s * x + c * y + dy, th + dth))
    return out


def chain_problem(pose_xyt, NL, b_pose, b_lm, b_z, lm_xy=None, odom_noise=None):
    """A valid bos.Problem over given poses and bearings: an odometry chain 0-1-2-... measured with
    O.predict_odometry (plus odom_noise, [NP - 1, 3]), the datasets' information, pose 0 fixed."""
    pose_xyt = np.ascontiguousarray(pose_xyt, dtype=np.float64)
    NP = len(pose_xyt)
    o_z = np.array([O.predict_odometry(pose_xyt[i], pose_xyt[i + 1]) for i in range(NP - 1)])
    if odom_noise is not None:
        o_z = o_z + odom_noise
    om = np.tile(np.diag([500.0, 500.0, 5000.0]), (NP - 1, 1, 1))
    return bos.Problem(pose_xyt, np.zeros((NL, 2)) if lm_xy is None else lm_xy, b_pose, b_lm, b_z,
                       np.arange(NP - 1, dtype=np.int32), np.arange(1, NP, dtype=np.int32), o_z, om, 0)


def _wrap(a):
    """a into [-pi, pi) (doubles; the world builders only)."""
    return (a + np.pi) % (2 * np.pi) - np.pi


def triangulation_case_world(seed=7):
    """The hand-made world of tests/test_gpu_triangulation_edges.py: (P, kinds). Every landmark is one
    case, kinds[l] = (kind, tag):
      rank2      M poses at distances 2-10 from the landmark within an angular spread (tag: set, spread,
                 M); sets: "plain", "far" (everything moved by (1e4, -1e4)), "wide+" / "wide-" (headings
                 with th + z in (pi, 2 pi) / (-2 pi, -pi)), "pool" (2-6 poses of a shared pool)
      one        a single observation (tag: "zero", "half_pi" or "random")
      none       no observation (the last landmark is one)
      par_a      exactly parallel rows, z in {0, pi/2, pi/4, 0.3}, M in {2, 3, 8}: poses with th = 0
      par_b      exactly parallel rows, z uniform in (-pi, pi), M in {2, 3, 7, 16}
      twice      one pose seen twice with two different z (rank 2: the pose's own position)
      twice_same one pose seen twice with the same z (exactly parallel)
    The bearings are in shuffled file order (the landmarks' lists interleave)."""
    rng = np.random.default_rng(seed)
    poses = [(0.0, 0.0, 0.0)]
    lms = []   # (kind, tag, [(pose, z)])

    def graded(name, spread, M):
        off = np.array([1e4, -1e4]) if name == "far" else np.zeros(2)
        L = rng.uniform(-5, 5, 2) + off
        # phi: direction pose -> landmark; psi = phi + pi: landmark -> pose
        phi0 = {"wide+": rng.uniform(-np.pi + 0.8, -0.8), "wide-": rng.uniform(0.8, np.pi - 0.8)}.get(
            name, rng.uniform(-np.pi, np.pi))
        u = rng.uniform(-0.5, 0.5, M)
        u[0], u[1] = -0.5, 0.5
        obs = []
        for i in range(M):
            psi, d = phi0 + np.pi + spread * u[i], rng.uniform(2, 10)
            p = L + d * np.array([np.cos(psi), np.sin(psi)])
            phi = np.arctan2(L[1] - p[1], L[0] - p[0])
            noise = 1e-3 * spread * rng.normal()
            if name == "wide+":      # th + z = phi + 2 pi in (pi, 2 pi)
                th = rng.uniform(phi + np.pi + 0.1, np.pi - 0.05)
                z = phi + 2 * np.pi - th + noise
            elif name == "wide-":    # th + z = phi - 2 pi in (-2 pi, -pi)
                th = rng.uniform(-np.pi + 0.05, phi - np.pi - 0.1)
                z = phi - 2 * np.pi - th + noise
            else:
                th = rng.uniform(-np.pi, np.pi)
                z = _wrap(phi - th + noise)
            assert -np.pi < z < np.pi and -np.pi <= th < np.pi
            poses.append((p[0], p[1], th))
            obs.append((len(poses) - 1, z))
        lms.append(("rank2", (name, spread, M), obs))

    for name in ("plain", "far", "wide+", "wide-"):
        for spread in (1.0, 1e-2, 1e-4, 1e-6):
            for M in (2, 3, 5, 17, 64, 65):
                graded(name, spread, M)
    # shared pool: random headings, landmarks seen by 2-6 of its poses
    pool = []
    for _ in range(40):
        poses.append((rng.uniform(-10, 10), rng.uniform(-10, 10), rng.uniform(-np.pi, np.pi)))
        pool.append(len(poses) - 1)
    for _ in range(110):
        L = rng.uniform(-15, 15, 2)
        obs = []
        for i in rng.choice(pool, rng.integers(2, 7), replace=False):
            x, y, th = poses[i]
            obs.append((int(i), _wrap(np.arctan2(L[1] - y, L[0] - x) - th + 1e-3 * rng.normal())))
        lms.append(("rank2", ("pool", 0.0, len(obs)), obs))
    # one observation
    for tag, th, z in [("zero", 0.0, 0.0), ("half_pi", 0.0, np.pi / 2)] + [("random", None, None)] * 10:
        if th is None:
            th, z = rng.uniform(-np.pi, np.pi), rng.uniform(-np.pi, np.pi)
        poses.append((rng.uniform(-10, 10), rng.uniform(-10, 10), th))
        lms.append(("one", tag, [(len(poses) - 1, z)]))
    # exactly parallel: 16 poses with th = 0 at different places, each landmark one z from the first M
    par = []
    for _ in range(16):
        poses.append((rng.uniform(-10, 10), rng.uniform(-10, 10), 0.0))
        par.append(len(poses) - 1)
    for z in (0.0, np.pi / 2, np.pi / 4, 0.3):
        for M in (2, 3, 8):
            lms.append(("par_a", (z, M), [(i, z) for i in par[:M]]))
    zb = np.random.default_rng(1234).uniform(-np.pi, np.pi, 64)
    for j, z in enumerate(zb):
        M = (2, 3, 7, 16)[j % 4]
        lms.append(("par_b", (float(z), M), [(i, float(z)) for i in par[:M]]))
    # one pose seen twice
    for dz in (1.0, 0.01, -2.0):
        i, z = int(rng.choice(pool)), rng.uniform(-1, 1)
        lms.append(("twice", dz, [(i, z), (i, z + dz)]))
    for _ in range(3):
        i, z = int(rng.choice(pool)), rng.uniform(-np.pi, np.pi)
        lms.append(("twice_same", None, [(i, z), (i, z)]))
    # no observation: three among the others, one last
    for _ in range(3):
        lms.append(("none", None, []))
    order = rng.permutation(len(lms))
    lms = [lms[i] for i in order] + [("none", None, [])]
    b = [(p, l, z) for l, (_, _, obs) in enumerate(lms) for p, z in obs]
    b = [b[i] for i in rng.permutation(len(b))]
    P = chain_problem(np.array(poses), len(lms), [p for p, _, _ in b], [l for _, l, _ in b], [z for _, _, z in b])
    return P, [(k, t) for k, t, _ in lms]


def corridor_world(seed=3, NP=300, sigma_z=1e-3, sigma_x0=0.02):
    """Poses one metre apart on the x axis whose true headings alternate between pi - 1e-3 and
    -pi + 1e-3, landmarks at y = +-3 each seen by 6 consecutive poses; measurements are the ground
    truth's predictions plus N(0, sigma_z), the initial guess the ground truth plus N(0, sigma_x0) on
    every component (theta wrapped into [-pi, pi)), pose 0 fixed at its ground truth. With sigma_x0
    twenty times the 1e-3 the headings keep from the wrap, about half the poses start on the far side
    of +-pi and one GN step brings them back across it."""
    rng = np.random.default_rng(seed)
    gt = np.zeros((NP, 3))
    gt[:, 0] = np.arange(NP)
    gt[0::2, 2] = np.pi - 1e-3
    gt[1::2, 2] = -np.pi + 1e-3
    NL = NP // 2
    gl = np.stack([2.0 * np.arange(NL) + 0.5, np.where(np.arange(NL) % 2 == 0, 3.0, -3.0)], axis=1)
    bp, bl = [], []
    for j in range(NL):
        for i in range(2 * j - 2, 2 * j + 4):
            if 0 <= i < NP:
                bp.append(i)
                bl.append(j)
    bz = np.array([O.predict_bearing(gt[i], gl[j]) for i, j in zip(bp, bl)]) + rng.normal(0, sigma_z, len(bp))
    x0 = gt + rng.normal(0, sigma_x0, gt.shape)
    x0[:, 2] = _wrap(x0[:, 2])
    x0[0] = gt[0]
    l0 = gl + rng.normal(0, sigma_x0, gl.shape)
    P = chain_problem(gt, NL, bp, bl, bz, odom_noise=rng.normal(0, sigma_z, (NP - 1, 3)))
    P.pose_xyt[:] = x0
    P.lm_xy[:] = l0
    P.gt_pose_xyt, P.gt_lm_xy = gt, gl
    return P


def rotated_world(P, alpha):
    """P turned rigidly by alpha about the origin: positions rotated, alpha added to the headings
    (wrapped); the measurements are relative and stay."""
    c, s = np.cos(alpha), np.sin(alpha)
    R = np.array([[c, -s], [s, c]])
    pose = P.pose_xyt.copy()
    pose[:, :2] = pose[:, :2] @ R.T
    pose[:, 2] = _wrap(pose[:, 2] + alpha)
    return bos.Problem(pose, P.lm_xy @ R.T, P.b_pose, P.b_lm, P.b_z, P.o_src, P.o_dst, P.o_z, P.o_omega, P.fixed,
                       b_omega=P.b_omega)
