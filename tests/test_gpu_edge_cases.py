"""Edge cases of the HIP J+H build and GN step against the CPU oracle, on variants of the
reference dataset (C1) and small synthetic worlds. Each case exercises a kernel path the
headline configs do not: duplicate (pose, landmark) observations (summed into one block, the
run-continuation flag), duplicate odometry pairs, poses with more than two odometry entries (loop
closures), odometry edges in both directions between the same poses (one shared pose-pose block
stored by the lower pose), odometry self-loops (zero Jacobian in the reference: chi^2 only),
bearing weights (HAS_W), poses without bearings and landmarks without observations (empty lanes),
two lanes per pose (dense poses), odd list lengths (the pair loop's tail), per-edge odometry
information (om_stride 6: every other case feeds one diagonal Omega, the om_stride 0 shortcut),
landmarks with 2047-4096 bearings (the packed landmark-lane header on both sides of its count's sign
bit, and the unpacked ll_lm / ll_cnt / ll_run arrays from 4096 on). Every GN step must report
solver_info == 0.

Tolerances as tests/test_gpu_parity.py: fp64 H within 1e-12 of max |H| (b 1e-11), fp32 within 2e-4;
state after 3 GN steps within rtol 1e-6 / atol 1e-9 of the oracle's."""
import numpy as np
import pytest

import bos
import oracle as O
from conftest import C1
from helpers import close_state, knife_edge_bearings, lin_parity, literal_oracle, to_oracle

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def c1():
    return bos.load_g2o(C1)


def _variant(P, **kw):
    a = dict(pose_xyt=P.pose_xyt, lm_xy=P.lm_xy, b_pose=P.b_pose, b_lm=P.b_lm, b_z=P.b_z, o_src=P.o_src,
             o_dst=P.o_dst, o_z=P.o_z, o_omega=P.o_omega, fixed=P.fixed, b_omega=P.b_omega,
             pose_ids=P.pose_ids, lm_ids=P.lm_ids)
    a.update(kw)
    return bos.Problem(**a)


def _dup_bearings(P, n=200, seed=1):
    rng = np.random.default_rng(seed)
    k = rng.choice(len(P.b_z), n, replace=False)
    return _variant(P, b_pose=np.concatenate([P.b_pose, P.b_pose[k]]), b_lm=np.concatenate([P.b_lm, P.b_lm[k]]),
                    b_z=np.concatenate([P.b_z, P.b_z[k] + rng.normal(0, 0.01, n)]))


def _dup_odometry(P, n=20, seed=2):
    rng = np.random.default_rng(seed)
    k = rng.choice(len(P.o_z), n, replace=False)
    return _variant(P, o_src=np.concatenate([P.o_src, P.o_src[k]]), o_dst=np.concatenate([P.o_dst, P.o_dst[k]]),
                    o_z=np.concatenate([P.o_z, P.o_z[k] + rng.normal(0, 0.02, (n, 3))]),
                    o_omega=np.concatenate([P.o_omega, P.o_omega[k]]))


def _loop_closures(P, n=30, gap=50, seed=3):
    """Edges (i, i + gap) measured from the current estimate plus noise: those poses get 3-4 entries."""
    rng = np.random.default_rng(seed)
    src = rng.choice(P.NP - gap, n, replace=False).astype(np.int32)
    dst = (src + gap).astype(np.int32)
    Q = to_oracle(P)
    z = np.zeros((n, 3))
    for i, (s, d) in enumerate(zip(src, dst)):
        z[i] = O.predict_odometry(Q.pose_xyt[s], Q.pose_xyt[d]) + rng.normal(0, 0.05, 3)
    return _variant(P, o_src=np.concatenate([P.o_src, src]), o_dst=np.concatenate([P.o_dst, dst]),
                    o_z=np.concatenate([P.o_z, z]), o_omega=np.concatenate([P.o_omega, P.o_omega[:n]]))


def _reversed_edges(P, n=25, seed=6):
    """Edges (d, s) added next to existing (s, d): g2o files hold such reversed loop closures, and
    the reference sums both into H(s, d) / H(d, s) (slam/solver.cpp:48-62)."""
    rng = np.random.default_rng(seed)
    k = rng.choice(len(P.o_z), n, replace=False)
    Q = to_oracle(P)
    src, dst = P.o_dst[k].astype(np.int32), P.o_src[k].astype(np.int32)
    z = np.array([O.predict_odometry(Q.pose_xyt[s], Q.pose_xyt[d]) for s, d in zip(src, dst)]) + rng.normal(0, 0.03, (n, 3))
    return _variant(P, o_src=np.concatenate([P.o_src, src]), o_dst=np.concatenate([P.o_dst, dst]),
                    o_z=np.concatenate([P.o_z, z]), o_omega=np.concatenate([P.o_omega, P.o_omega[k]]))


def _self_loops(P, n=7, seed=7):
    """Odometry edges (i, i): their Jacobian is zero in the reference (the two 3x3 blocks land on
    the same columns and cancel exactly), so they add chi^2 (and may trip the robust count) only."""
    rng = np.random.default_rng(seed)
    p = rng.choice(P.NP, n, replace=False).astype(np.int32)
    z = rng.normal(0, 0.05, (n, 3))
    z[0] = (2.0, -1.0, 0.5)   # rho far above the kernel threshold
    return _variant(P, o_src=np.concatenate([P.o_src, p]), o_dst=np.concatenate([P.o_dst, p]),
                    o_z=np.concatenate([P.o_z, z]), o_omega=np.concatenate([P.o_omega, P.o_omega[:n]]))


def _weights(P, seed=4):
    rng = np.random.default_rng(seed)
    return _variant(P, b_omega=rng.uniform(0.5, 2.0, len(P.b_z)))


def _poses_without_bearings(P, n=20, seed=5):
    """All bearings of n poses dropped: empty pose lanes, and landmarks seen only by those poses
    keep no observation at all (empty landmark lanes; damping keeps H positive definite)."""
    rng = np.random.default_rng(seed)
    cand = np.setdiff1d(np.arange(P.NP), [P.fixed])
    drop = rng.choice(cand, n, replace=False)
    keep = ~np.isin(P.b_pose, drop)
    return _variant(P, b_pose=P.b_pose[keep], b_lm=P.b_lm[keep], b_z=P.b_z[keep])


def _information(n, seed=21):
    """n SPD odometry information matrices with off-diagonals, Omega_k = D (A_k A_k^T + I) D with A_k ~
    N(0, 1) 3 x 3 and D = diag(sqrt 500, sqrt 500, sqrt 5000): the scale of the datasets' diagonal one."""
    A = np.random.default_rng(seed).normal(0, 1, (n, 3, 3))
    D = np.diag(np.sqrt([500.0, 500.0, 5000.0]))
    return D @ (A @ A.transpose(0, 2, 1) + np.eye(3)) @ D


def _varied_information(P):
    return _variant(P, o_omega=_information(len(P.o_z)))


CASES = {
    "dup_bearings": _dup_bearings,
    "dup_odometry": _dup_odometry,
    "loop_closures": _loop_closures,
    "weights": _weights,
    "poses_without_bearings": _poses_without_bearings,
    "reversed_edges": _reversed_edges,
    "self_loops": _self_loops,
    "everything": lambda P: _self_loops(_reversed_edges(_weights(_loop_closures(_dup_odometry(_dup_bearings(
        _poses_without_bearings(P))))))),
    "varied_information": _varied_information,
    "everything_varied": lambda P: _self_loops(_reversed_edges(_weights(_loop_closures(_dup_odometry(_dup_bearings(
        _varied_information(_poses_without_bearings(P)))))))),
}


def _steps_match(P, precision=bos.BOS_FP64, n=3, rtol=1e-6):
    Q = to_oracle(P)
    S = bos.Solver(P, precision=precision)
    chis = []
    for _ in range(n):
        st = S.step()
        assert st["solver_info"] == 0
        chis.append(st["chi2"])
    pg, lg = S.get_state()
    S.close()
    po, lo = Q.copy_state()
    with literal_oracle(P):
        for i in range(n):
            c, _, _ = O.step(Q, po, lo)
            assert abs(chis[i] - c) <= 1e-9 * max(c, 1.0), (i, chis[i], c)
    return close_state(pg, lg, po, lo, rtol=rtol)


@pytest.mark.parametrize("case", sorted(CASES))
def test_edge_case_linearize_fp64(c1, case):
    lin_parity(CASES[case](c1))


@pytest.mark.parametrize("case", ["dup_bearings", "everything", "varied_information", "everything_varied"])
def test_edge_case_linearize_fp32(c1, case):
    lin_parity(CASES[case](c1), precision=bos.BOS_FP32, tol=2e-4, btol=2e-3)


@pytest.mark.parametrize("case", sorted(CASES))
def test_edge_case_steps(c1, case):
    ok, dp, dl = _steps_match(CASES[case](c1))
    assert ok, (dp, dl)


def test_two_lanes_per_pose():
    """Poses with >= 32 bearings on average run two lanes per pose (lane-group butterfly)."""
    P = bos.synthetic(300, 3000, 40, seed=11)
    assert bos.plan_inspect(P, 0, 1)["lanes_per_pose"] == 2
    lin_parity(P)
    ok, dp, dl = _steps_match(P)
    assert ok, (dp, dl)


def test_odd_list_lengths():
    """Every pose with an odd number of bearings: the pair loop's last item runs alone and its
    block goes to the lane's padding slot."""
    P = bos.synthetic(400, 1200, 9, seed=12)
    assert np.all(np.bincount(P.b_pose, minlength=P.NP) % 2 == 1)
    lin_parity(P)


# ---------------------------------------------------------------- per-edge odometry information
@pytest.fixture(scope="module")
def varied_world():
    """synthetic(200, 300, 8) with every pose but the fixed one moved by N(0, 0.02) and per-edge
    information. The perturbation matters: at the generator's initial guess (the dead-reckoned
    odometry chain) the odometry errors are ~0, and then neither b nor chi^2 can see Omega."""
    P = bos.synthetic(200, 300, 8, seed=5)
    d = np.random.default_rng(8).normal(0, 0.02, P.pose_xyt.shape)
    d[P.fixed] = 0.0
    P = _variant(P, pose_xyt=P.pose_xyt + d, o_omega=_information(len(P.o_z)))
    assert len(knife_edge_bearings(P)[0]) == 0
    return P


def test_varied_information_linearize_fp64(varied_world):
    with O.literal():
        chi = O.linearize(to_oracle(varied_world)).chi2
    assert chi > 1000.0   # the odometry residuals are not ~0: Omega shows in b and chi^2
    lin_parity(varied_world)


def test_varied_information_linearize_fp32(varied_world):
    lin_parity(varied_world, precision=bos.BOS_FP32, tol=2e-4, btol=2e-3)


def test_varied_information_steps(varied_world):
    ok, dp, dl = _steps_match(varied_world)
    assert ok, (dp, dl)


def test_information_stride_0_equals_stride_6():
    """A uniform-Omega world (one information row on the device, om_stride 0) and the same world plus
    one self-loop (p, p) with another Omega (solver_create.hip then keeps a row per edge, om_stride 6).
    A self-loop has a zero Jacobian and is kept aside of the lanes, and p, one end of a loop closure, is
    off the odometry-chain shortcut in both worlds, so the lane layout is the same: H and b must agree
    bit for bit, and chi^2 differ by the self-loop's e^T Omega e."""
    P = bos.synthetic(200, 300, 8, seed=5)
    assert np.all(P.o_omega == P.o_omega[0])
    p, q = 60, 140
    z = O.predict_odometry(P.pose_xyt[p], P.pose_xyt[q]) + np.array([0.03, -0.02, 0.01])
    U = _variant(P, o_src=np.concatenate([P.o_src, [p]]), o_dst=np.concatenate([P.o_dst, [q]]),
                 o_z=np.concatenate([P.o_z, z[None]]), o_omega=np.concatenate([P.o_omega, P.o_omega[:1]]))
    zl, om = np.array([0.3, -0.2, 0.1]), _information(1, seed=22)
    V = _variant(U, o_src=np.concatenate([U.o_src, [p]]), o_dst=np.concatenate([U.o_dst, [p]]),
                 o_z=np.concatenate([U.o_z, zl[None]]), o_omega=np.concatenate([U.o_omega, om]))
    assert bos.plan_inspect(U)["pose_odometry_chain"] == bos.plan_inspect(V)["pose_odometry_chain"] == P.NP - 2 - 2
    term = float(zl @ om[0] @ zl)   # e = 0 - z (|z_theta| < pi: no wrap)
    for precision in (bos.BOS_FP64, bos.BOS_FP32):
        out = []
        for W in (U, V):
            S = bos.Solver(W, precision=precision)
            st = S.linearize()
            out.append((st, S.export_system()))
            S.close()
        (su, eu), (sv, ev) = out
        for a, b in zip(eu, ev):
            assert np.array_equal(a, b)
        assert sv["n_robust"] == su["n_robust"] + 1
        # the sum's order may differ: n eps sum |terms| with n ~ 2000 observations is ~2e-13 chi^2 in fp64
        tol = 1e-11 if precision == bos.BOS_FP64 else 1e-3
        assert abs(sv["chi2"] - su["chi2"] - term) <= tol * max(sv["chi2"], 1.0), (sv["chi2"], su["chi2"], term)
    lin_parity(V)


# ---------------------------------------------------------------- landmark-lane headers
_lane_worlds = {}


def _lane_world(n):
    """synthetic(40, 40, 4) with bearings of landmark 0 from poses 8..23 (ground truth plus N(0, 0.01))
    added until it has exactly n: 256-long duplicate (pose, landmark) runs on the pose side too."""
    if n not in _lane_worlds:
        P = bos.synthetic(40, 40, 4, seed=5)
        add = n - int(np.sum(P.b_lm == 0))
        assert add > 0
        rng = np.random.default_rng(3)
        pose = (8 + np.arange(add) % 16).astype(np.int32)
        z = np.array([O.predict_bearing(P.gt_pose_xyt[i], P.gt_lm_xy[0]) for i in pose]) + rng.normal(0, 0.01, add)
        W = _variant(P, b_pose=np.concatenate([P.b_pose, pose]), b_lm=np.concatenate([P.b_lm, np.zeros(add, np.int32)]),
                     b_z=np.concatenate([P.b_z, z]))
        assert int(np.sum(W.b_lm == 0)) == n and len(knife_edge_bearings(W)[0]) == 0
        _lane_worlds[n] = W
    return _lane_worlds[n]


LANE_COUNTS = [2047, 2048, 4095, 4096]   # packed header below / at the count's sign bit (bit 31), its last count, unpacked


@pytest.mark.parametrize("n", LANE_COUNTS)
def test_landmark_lane_header_linearize_fp64(n):
    lin_parity(_lane_world(n))


@pytest.mark.parametrize("n", LANE_COUNTS)
def test_landmark_lane_header_linearize_fp32(n):
    lin_parity(_lane_world(n), precision=bos.BOS_FP32, tol=2e-4, btol=2e-3)


@pytest.mark.parametrize("n", LANE_COUNTS)
def test_landmark_lane_header_steps(n):
    ok, dp, dl = _steps_match(_lane_world(n))
    assert ok, (dp, dl)
