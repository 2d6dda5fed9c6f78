"""Reference of the prior-factor tests (test_priors_host.py, test_gpu_priors.py): the terms of a pose
prior and of a landmark prior in NumPy fp64, transcribed operation by operation from the comment of
bos_set_priors (include/bos.h), and GN steps / costs with priors on top of the CPU oracle
(O.linearize, O.assemble_H, O.solve_dx, O.apply_boxplus). No code shared with the product.

A prior set is a dict {"pose": (index, mean [n, 3], omega [n, 3, 3]) or None,
"landmark": (index, mean [n, 2], omega [n, 2, 2]) or None}."""
import numpy as np
import scipy.sparse as sp

import lm_ref
import oracle as O

F = np.float64
PI, TWO_PI = F(O.CV_PI), F(6.283185307179586476925286766559)


def normalized_angle(a):
    """[-pi, pi): the reference's loops (|a| stays far below the product's 1e6 shortcut here)."""
    a = F(a)
    while a < -PI:
        a = F(a + TWO_PI)
    while a >= PI:
        a = F(a - TWO_PI)
    return a


def pose_terms(state, mean, omega):
    """(A [6] = (00, 10, 11, 20, 21, 22), g [3], rho, e [3]) of a pose prior; one operation per step."""
    x, y, th = (F(v) for v in state)
    m0, m1, m2 = (F(v) for v in mean)
    om = np.asarray(omega, dtype=F).reshape(3, 3)
    u00, u01, u02, u11, u12, u22 = om[0, 0], om[0, 1], om[0, 2], om[1, 1], om[1, 2], om[2, 2]
    e0, e1 = F(x - m0), F(y - m1)
    e2 = normalized_angle(F(th - m2))
    Oe0 = F(F(F(u00 * e0) + F(u01 * e1)) + F(u02 * e2))
    Oe1 = F(F(F(u01 * e0) + F(u11 * e1)) + F(u12 * e2))
    Oe2 = F(F(F(u02 * e0) + F(u12 * e1)) + F(u22 * e2))
    rho = F(F(F(e0 * Oe0) + F(e1 * Oe1)) + F(e2 * Oe2))
    ny = F(-y)
    g = np.array([Oe0, Oe1, F(F(F(ny * Oe0) + F(x * Oe1)) + Oe2)], dtype=F)
    q0 = F(F(F(ny * u00) + F(x * u01)) + u02)
    q1 = F(F(F(ny * u01) + F(x * u11)) + u12)
    q2 = F(F(F(ny * u02) + F(x * u12)) + u22)
    A = np.array([u00, u01, u11, q0, q1, F(F(F(ny * q0) + F(x * q1)) + q2)], dtype=F)
    return A, g, float(rho), np.array([e0, e1, e2], dtype=F)


def landmark_terms(state, mean, omega):
    """(A [3] = (00, 10, 11), g [2], rho, e [2]) of a landmark prior."""
    lx, ly = (F(v) for v in state)
    m0, m1 = (F(v) for v in mean)
    om = np.asarray(omega, dtype=F).reshape(2, 2)
    u00, u01, u11 = om[0, 0], om[0, 1], om[1, 1]
    e0, e1 = F(lx - m0), F(ly - m1)
    g0 = F(F(u00 * e0) + F(u01 * e1))
    g1 = F(F(u01 * e0) + F(u11 * e1))
    rho = F(F(e0 * g0) + F(e1 * g1))
    return np.array([u00, u01, u11], dtype=F), np.array([g0, g1], dtype=F), float(rho), np.array([e0, e1], dtype=F)


def pose_jacobian(state):
    x, y = float(state[0]), float(state[1])
    return np.array([[1.0, 0.0, -y], [0.0, 1.0, x], [0.0, 0.0, 1.0]])


def tri_to_full(A):
    """Lower triangle in the block array's order -> symmetric matrix."""
    d = 3 if len(A) == 6 else 2
    M = np.zeros((d, d))
    k = 0
    for i in range(d):
        for j in range(i + 1):
            M[i, j] = M[j, i] = A[k]
            k += 1
    return M


def each(priors, NP):
    """(kind, node, first dof, dim, mean, omega) of every prior: pose priors, then landmark priors."""
    out = []
    for kind, dim in (("pose", 3), ("landmark", 2)):
        pr = (priors or {}).get(kind)
        if pr is None:
            continue
        idx = np.asarray(pr[0], dtype=np.int64).reshape(-1)
        mean = np.asarray(pr[1], dtype=F).reshape(len(idx), dim)
        om = np.asarray(pr[2], dtype=F).reshape(len(idx), dim, dim)
        for i, node in enumerate(idx):
            dof = 3 * int(node) if kind == "pose" else 3 * NP + 2 * int(node)
            out.append((kind, int(node), dof, dim, mean[i], om[i]))
    return out


def terms(priors, NP, pose, lm):
    """Per prior (kind, node, dof, dim, A full [dim, dim], g, rho, e, mean, omega) at a state."""
    out = []
    for kind, node, dof, dim, mean, om in each(priors, NP):
        if kind == "pose":
            A, g, rho, e = pose_terms(pose[node], mean, om)
        else:
            A, g, rho, e = landmark_terms(lm[node], mean, om)
        out.append((kind, node, dof, dim, tri_to_full(A), g, rho, e, mean, om))
    return out


def add_priors(Q, H, b, priors, pose, lm):
    """(H + sum A, b + sum g, sum rho) with H a scipy matrix in the reference dof order."""
    H = sp.lil_matrix(H)
    b = np.array(b, dtype=F)
    total = 0.0
    for _, _, dof, dim, A, g, rho, _, _, _ in terms(priors, Q.NP, pose, lm):
        H[dof:dof + dim, dof:dof + dim] = H[dof:dof + dim, dof:dof + dim].toarray() + A
        b[dof:dof + dim] += g
        total += rho
    return H.tocsr(), b, total


def sum_rho(priors, NP, pose, lm):
    return float(sum(t[6] for t in terms(priors, NP, pose, lm)))


def step(Q, pose, lm, priors, kernel_threshold=1.0, damping=0.01):
    """One GN step with priors in place: (chi2 with the priors' rho, dx)."""
    lin = O.linearize(Q, pose, lm, kernel_threshold, damping)
    H, b, rho = add_priors(Q, O.assemble_H(Q, lin), lin.b, priors, pose, lm)
    dx = O.solve_dx(Q, H, b)
    O.apply_boxplus(Q, pose, lm, dx)
    return lin.chi2 + rho, dx


def cost(Q, pose, lm, kt, priors):
    """(F, chi2, n_robust) at a state: lm_ref.cost plus the priors' rho (not robustified) in both sums."""
    Fv, chi, nrob = lm_ref.cost(Q, pose, lm, kt)
    r = sum_rho(priors, Q.NP, pose, lm)
    return Fv + r, chi + r, nrob


def random_priors(P, n_pose, n_landmark, seed, sigma=0.3, spread=0.2, exclude_pose=()):
    """A deterministic mixed prior set near the problem's state: random nodes (never the fixed pose), means
    within `spread` of the state (|theta - m2| far below 3), random SPD informations of scale 1 / sigma^2."""
    rng = np.random.default_rng(seed)
    free = np.array([p for p in range(P.NP) if p != P.fixed and p not in set(exclude_pose)])
    pi = np.sort(rng.choice(free, size=min(n_pose, len(free)), replace=False))
    li = np.sort(rng.choice(P.NL, size=min(n_landmark, P.NL), replace=False))

    def spd(n, d):
        M = rng.normal(size=(n, d, d))
        S = M @ np.transpose(M, (0, 2, 1)) + d * np.eye(d)
        S = S / sigma ** 2
        return 0.5 * (S + np.transpose(S, (0, 2, 1)))   # bit-symmetric

    return {"pose": (pi.astype(np.int32), P.pose_xyt[pi] + spread * rng.uniform(-1, 1, (len(pi), 3)), spd(len(pi), 3)),
            "landmark": (li.astype(np.int32), P.lm_xy[li] + spread * rng.uniform(-1, 1, (len(li), 2)), spd(len(li), 2))}
