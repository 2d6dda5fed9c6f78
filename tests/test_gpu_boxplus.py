"""boxplus_kernel in isolation: the state after one GN step must be the box-plus of the state before it
with the applied update (bos_get_last_dx), evaluated at 50 digits from the exact doubles
(helpers.mp_boxplus). Every other test sees the kernel only through whole GN steps compared with the
oracle's within rtol 1e-6, which a wrong wrap at +-pi, a touched fixed pose or a wrong max_abs_dx
could survive.

Per pose, x' = cos(dth) x - sin(dth) y + dx, y' = sin(dth) x + cos(dth) y + dy, th' = th + dth:
  positions  |x1 - x'|, |y1 - y'| <= 8 eps (|x0| + |y0| + |d|): the device sin / cos within 2 ulp, two
             products, two additions, a possible fused multiply-add;
  theta      circular distance of th1 to th' <= 8 eps (one rounding of the sum, one of the +-2 pi
             shift, the error of the double 2 pi: under 7e-16 together), and -pi <= th1 < pi against
             the double pi;
  fixed pose bit-identical, its dx entries 0;
  landmarks  lm1 == lm0 + dx bit for bit (one addition);
  max_abs_dx == max |dx| exactly.

Worlds: the reference dataset, bos.synthetic(300, 300, 8, seed=5), and helpers.corridor_world, whose
headings sit 1e-3 from +-pi so that dozens of poses cross the wrap in one step, in both directions
(counted from the oracle's own step). The corridor's three-step state is also compared with the
oracle's, and one whole step is checked for covariance under a rigid rotation of the world.

Measured on an MI355X (each test prints its own): positions at most 0.12 of their bound, theta at most
0.26 of 8 eps (the corridor; 0.125 elsewhere), fp64 and fp32 handles alike. Without the `>= pi` loop of
normalized_angle the [-pi, pi) assertion fails on the corridor and the reference dataset; with the sign
of sin(dth) flipped the position bound fails on every world (tried on the device, not kept)."""
import mpmath as mp
import numpy as np
import pytest

import bos
import oracle as O
from conftest import C1
from helpers import EPS, close_state, corridor_world, knife_edge_bearings, literal_oracle, mp_boxplus, rotated_world, to_oracle

pytestmark = pytest.mark.gpu

_worlds = {}


def _world(name):
    if name not in _worlds:
        _worlds[name] = {"c1": lambda: bos.load_g2o(C1), "synthetic": lambda: bos.synthetic(300, 300, 8, seed=5),
                         "corridor": lambda: corridor_world(seed=2)}[name]()
    return _worlds[name]


def _one_step(P, precision):
    S = bos.Solver(P, precision=precision)
    pose0, lm0 = S.get_state()
    st = S.step()
    assert st["solver_info"] == 0
    dx = S.last_dx()
    pose1, lm1 = S.get_state()
    S.close()
    return pose0, lm0, st, dx, pose1, lm1


def _check_boxplus(P, pose0, lm0, dx, pose1, lm1, label):
    """state1 == state0 [+] dx by the module docstring's bounds."""
    dp, dl = dx[:3 * P.NP].reshape(-1, 3), dx[3 * P.NP:].reshape(-1, 2)
    assert np.all(np.isfinite(dx)) and np.abs(dp[:, 2]).max() > 0
    # the fixed pose
    assert np.array_equal(pose1[P.fixed], pose0[P.fixed]) and np.all(dp[P.fixed] == 0.0)
    # landmarks: one addition
    assert np.array_equal(lm1, lm0 + dl), np.abs(lm1 - (lm0 + dl)).max()
    # poses against the 50-digit box-plus
    pi = mp.pi
    worst_xy = worst_th = 0.0
    for i, (xr, yr, tr) in enumerate(mp_boxplus(pose0, dp)):
        if i == P.fixed:
            continue
        base = abs(pose0[i, 0]) + abs(pose0[i, 1])
        ex = abs(mp.mpf(float(pose1[i, 0])) - xr) / (8 * EPS * (base + abs(dp[i, 0])))
        ey = abs(mp.mpf(float(pose1[i, 1])) - yr) / (8 * EPS * (base + abs(dp[i, 1])))
        worst_xy = max(worst_xy, float(ex), float(ey))
        et = abs((mp.mpf(float(pose1[i, 2])) - tr + pi) % (2 * pi) - pi)
        worst_th = max(worst_th, float(et / (8 * EPS)))
    print(f"boxplus {label}: worst position error / bound {worst_xy:.3f}, worst theta error / (8 eps) {worst_th:.3f}")
    assert worst_xy <= 1.0
    assert worst_th <= 1.0
    assert np.all(pose1[:, 2] >= -np.pi) and np.all(pose1[:, 2] < np.pi)


@pytest.mark.parametrize("precision", [bos.BOS_FP64, bos.BOS_FP32])
@pytest.mark.parametrize("name", ["c1", "synthetic", "corridor"])
def test_state_is_boxplus_of_last_dx(name, precision):
    P = _world(name)
    assert P.NP + P.NL > 256                      # more than one update block
    pose0, lm0, st, dx, pose1, lm1 = _one_step(P, precision)
    _check_boxplus(P, pose0, lm0, dx, pose1, lm1, f"{name} precision {precision}")
    assert st["max_abs_dx"] == np.abs(dx).max()
    if name == "corridor":   # the device's own step crosses the wrap in both directions, as the oracle's
        s = pose0[:, 2] + dx[2:3 * P.NP:3]
        assert (s >= np.pi).sum() >= 20 and (s < -np.pi).sum() >= 20


def test_corridor_crosses_the_wrap_and_matches_oracle():
    """The oracle's own first step takes >= 20 poses up across +pi and >= 20 down across -pi; the
    product's state after three steps equals the oracle's (rtol 1e-6, as tests/test_gpu_edge_cases.py),
    which pins the wrap end to end."""
    P = _world("corridor")
    assert len(knife_edge_bearings(P)[0]) == 0
    assert P.NP + P.NL > 256
    Q = to_oracle(P)
    po, lo = Q.copy_state()
    S = bos.Solver(P)
    with literal_oracle(P):
        for i in range(3):
            th0 = po[:, 2].copy()
            c, _, dxo = O.step(Q, po, lo)
            if i == 0:
                s = th0 + dxo[2:3 * P.NP:3]
                print(f"corridor: oracle step crosses +pi {int((s >= np.pi).sum())} times, -pi {int((s < -np.pi).sum())} times")
                assert (s >= np.pi).sum() >= 20 and (s < -np.pi).sum() >= 20
            st = S.step()
            assert st["solver_info"] == 0
            assert abs(st["chi2"] - c) <= 1e-9 * max(c, 1.0), (i, st["chi2"], c)
    pg, lg = S.get_state()
    S.close()
    ok, dp, dl = close_state(pg, lg, po, lo, rtol=1e-6)
    assert ok, (dp, dl)


def test_step_is_covariant_under_rotation():
    """The synthetic world turned rigidly by 2.5 rad about the origin (measurements unchanged): with
    v2t(dx') R_a X = R_a v2t(R_a^T dx_t, dth) X the GN update is the same one expressed in the turned
    frame (the damping is isotropic), so dx' turned back and chi^2 equal the plain world's within the
    bounds of two solves of one system (1e-8 max |dx|, 1e-9 chi^2), and the new state is the plain
    world's new state turned."""
    alpha = 2.5
    P = _world("synthetic")
    Pr = rotated_world(P, alpha)
    assert len(knife_edge_bearings(P)[0]) == 0 and len(knife_edge_bearings(Pr)[0]) == 0
    _, _, st, dx, pose1, lm1 = _one_step(P, bos.BOS_FP64)
    _, _, str_, dxr, pose1r, lm1r = _one_step(Pr, bos.BOS_FP64)
    assert abs(str_["chi2"] - st["chi2"]) <= 1e-9 * st["chi2"]
    assert str_["n_robust"] == st["n_robust"]
    c, s = np.cos(alpha), np.sin(alpha)
    R = np.array([[c, -s], [s, c]])
    back = dxr.copy()
    dpr, dlr = back[:3 * P.NP].reshape(-1, 3), back[3 * P.NP:].reshape(-1, 2)
    dpr[:, :2] = dpr[:, :2] @ R       # rows times R: R^T applied to each vector
    dlr[:] = dlr @ R
    assert np.abs(back - dx).max() <= 1e-8 * np.abs(dx).max(), np.abs(back - dx).max() / np.abs(dx).max()
    want = pose1.copy()
    want[:, :2] = pose1[:, :2] @ R.T
    want[:, 2] = (pose1[:, 2] + alpha + np.pi) % (2 * np.pi) - np.pi
    ok, ep, el = close_state(pose1r, lm1r, want, lm1 @ R.T, rtol=1e-6)
    assert ok, (ep, el)
