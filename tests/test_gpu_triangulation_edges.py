"""triangulate_kernel (bos_triangulate, and bos_create with landmark_xy = NULL) on a hand-made world of
edge cases, against a 50-digit mpmath solution of the exact double inputs (helpers.mp_triangulate).
tests/test_gpu_triangulation.py runs the kernel on well-conditioned rank-2 landmarks and single
observations only; here every landmark of helpers.triangulation_case_world is one case:

  rank 2 at graded parallax (angular spread 1 .. 1e-6 rad, kappa_2 1 .. 4e6; M = 2 .. 65 rows), plain,
  moved by (1e4, -1e4) (cancellation in the right-hand side), and with th + z in (pi, 2 pi) and
  (-2 pi, -pi); landmarks seen from a shared pose pool; both pivot choices; M = 1; M = 0 (the last
  landmark among them); exactly parallel rows with M >= 2 (the rank rule's `rem < thr` branch); one
  pose seen twice. 304 landmarks: two blocks, the last partial; the bearings' file order is shuffled, so
  bos_create's grouping by landmark is exercised too.

Bounds. Rank 2: |xy - xy_ref|_inf <= C kappa_2 eps scale, scale = max(1, max |p_xy| of the landmark's
poses, |xy_ref|_inf), kappa_2 from the 50-digit Gram matrix; C = 16 for the device, and C = 8 is
required of the CPU oracle on the same landmarks (a guard on the inputs). Basic solutions (M = 1,
parallel rows): the pivot column is the one of larger norm (the first on a tie), x_piv = (c.r)/(c.c)
within 16 eps scale, the other component exactly 0.0. The column norms are read off the 50-digit rows;
where they agree to (8 + M) eps (sin and cos within 2 ulp each, squared, M additions: only z = pi/4
here) the doubles cannot tell which is larger and either basic solution is accepted, each in full.

The exactly parallel landmarks with random z (par_b) are compared with the 50-digit basic solution
only, not with the oracle: the oracle restates Eigen's Householder rank rule, which is knife-edged on
exact rank-1 input (in a CPU probe of 1 800 such systems it chose rank 2 on 241 and returned
coordinates ~1e15; on this world's 64 it does so on 7), while the product's Gram-Schmidt rule chose
rank 1 on all of them. On the 12 par_a landmarks the oracle does return the basic solution, which the
guard test asserts.

Worst ratios measured on an MI355X (error / (kappa_2 eps scale) for rank 2, error / (eps scale) for
basic solutions; each test prints its own), fp64 and fp32 handles alike:
  rank 2 (bound 16):           device 2.148 at bos_create, 1.396 after set_state + bos_triangulate
  rank 2, oracle (bound 8):    2.369 and 1.424 on the same two states
  basic solutions (bound 16):  device 0.547 and 2.411
The device chose rank 1 on every exactly parallel landmark. With the second Gram-Schmidt pass
removed, or with the pivot choice inverted, the rank-2 ratios reach 1e6 and more and basic solutions
are missed (tried on the device, not kept)."""
import mpmath as mp
import numpy as np
import pytest

import bos
import oracle as O
from helpers import EPS, landmark_observations, mp_triangulate, triangulation_case_world

pytestmark = pytest.mark.gpu

C_DEVICE, C_ORACLE, C_BASIC = 16.0, 8.0, 16.0
RANK2 = ("rank2", "twice")
BASIC = ("one", "par_a", "par_b", "twice_same")


@pytest.fixture(scope="module")
def world():
    """(P, kinds, states): states[0] is P's poses, states[1] the same world shrunk by 1/2 and moved by
    (3, -2) (directions, hence z and every case's kind, stay; positions and right-hand sides do not),
    each with its 50-digit reference. Computed once, never modified."""
    P, kinds = triangulation_case_world()
    pose2 = P.pose_xyt * np.array([0.5, 0.5, 1.0]) + np.array([3.0, -2.0, 0.0])
    return P, kinds, [(pose, mp_triangulate(P, pose)) for pose in (P.pose_xyt.copy(), pose2)]


def _err(got, want):
    return max(abs(mp.mpf(float(got[0])) - want[0]), abs(mp.mpf(float(got[1])) - want[1]))


def _scale(d, want):
    return max(1.0, d["pmax"], abs(float(want[0])), abs(float(want[1])))


def _basic_ratio(got, d):
    """error / (eps scale) of got against the basic solution of d's pivot column (the better of the two
    where the column norms are indistinguishable in double), inf unless the other component is 0.0."""
    first = 1 if d["n1"] > d["n0"] else 0
    cand = [first]
    if abs(d["n0"] - d["n1"]) <= (8 + d["M"]) * EPS * max(d["n0"], d["n1"]):
        cand.append(1 - first)
    best = np.inf
    for c in cand:
        want = d["basic"][c]
        if float(got[1 - c]) == 0.0:
            best = min(best, float(_err(got, want) / (EPS * _scale(d, want))))
    return best


def _ratios(xy, kinds, ref):
    """Per landmark: error / (kappa_2 eps scale) (rank 2), error / (eps scale) (basic), 0 or inf (M = 0)."""
    out = np.zeros(len(kinds))
    for l, ((kind, _), d) in enumerate(zip(kinds, ref)):
        if kind in RANK2:
            out[l] = float(_err(xy[l], d["xy"]) / (d["kappa"] * EPS * _scale(d, d["xy"])))
        elif kind in BASIC:
            out[l] = _basic_ratio(xy[l], d)
        else:
            out[l] = 0.0 if (xy[l, 0] == 0.0 and xy[l, 1] == 0.0) else np.inf
    return out


def _check(xy, kinds, ref, c_rank2, label):
    r = _ratios(xy, kinds, ref)
    kind = np.array([k for k, _ in kinds])
    r2, rb, r0 = np.isin(kind, RANK2), np.isin(kind, BASIC), kind == "none"
    print(f"triangulation {label}: worst rank-2 ratio {r[r2].max():.3f} (bound {c_rank2}), "
          f"worst basic ratio {r[rb].max():.3f} (bound {C_BASIC})")
    bad = [(l, kinds[l], r[l], xy[l].tolist()) for l in np.nonzero((r2 & (r > c_rank2)) | (rb & (r > C_BASIC)) | (r0 & (r > 0)))[0]]
    assert not bad, bad[:8]
    return r


def _oracle_tri(P, pose):
    ids, xy = O.triangulate(pose, P.b_pose, np.arange(P.NL, dtype=np.int32)[P.b_lm], P.b_z)
    out = np.zeros((P.NL, 2))
    out[ids] = xy
    return out


def test_world_guards(world):
    """The inputs are what the cases claim, judged from the 50-digit rows and the CPU oracle alone."""
    P, kinds, states = world
    kind = np.array([k for k, _ in kinds])
    counts = np.bincount(P.b_lm, minlength=P.NL)
    assert P.NL >= 300 and P.NL % 256 != 0
    assert kinds[-1][0] == "none" and (kind == "none").sum() >= 4 and np.all(counts[kind == "none"] == 0)
    assert (kind == "one").sum() >= 8 and np.all(counts[kind == "one"] == 1)
    assert {t for k, t in kinds if k == "one"} >= {"zero", "half_pi"}
    assert (kind == "par_a").sum() == 12 and (kind == "par_b").sum() == 64
    # every rank-2 set at every spread and M
    tags = {t for k, t in kinds if k == "rank2"}
    assert all((n, s, M) in tags for n in ("plain", "far", "wide+", "wide-") for s in (1.0, 1e-2, 1e-4, 1e-6)
               for M in (2, 3, 5, 17, 64, 65))
    # the landmarks' bearings interleave in the file
    assert np.count_nonzero(np.diff(P.b_lm) != 0) > 0.9 * len(P.b_lm)
    obs = landmark_observations(P)
    for pose, ref in states:
        ang = pose[P.b_pose, 2] + P.b_z
        for l, (k, t) in enumerate(kinds):
            if k == "rank2" and t[0] == "wide+":
                assert np.all((ang[obs[l]] > np.pi) & (ang[obs[l]] < 2 * np.pi))
            if k == "rank2" and t[0] == "wide-":
                assert np.all((ang[obs[l]] < -np.pi) & (ang[obs[l]] > -2 * np.pi))
            if k in ("par_a", "par_b", "twice_same"):   # bit-identical rows
                assert len(set(zip(pose[P.b_pose[obs[l]], 2].tolist(), P.b_z[obs[l]].tolist()))) == 1
        # both pivot choices, and no rank-2 landmark in the ambiguous band of the rank rule
        n1_larger = np.array([d["M"] > 0 and d["n1"] > d["n0"] for d in ref])
        assert n1_larger.sum() >= 10 and (~n1_larger & (counts > 0)).sum() >= 10
        for basic in (True, False):
            sel = np.isin(kind, BASIC) if basic else np.isin(kind, RANK2)
            assert (n1_larger & sel).sum() >= 10 and (~n1_larger & sel).sum() >= 10
        kap = np.array([float(d["kappa"]) for (k, _), d in zip(kinds, ref) if k in RANK2])
        assert kap.min() < 1.5 and 1e6 < kap.max() < 1e8
        # the oracle: within C = 8 on the rank-2 landmarks, the basic solution on M = 1, the 12 par_a
        # and the twice-seen poses; par_b is not asked of it (module docstring)
        oxy = _oracle_tri(P, pose)
        r = _ratios(oxy, kinds, ref)
        print(f"oracle: worst rank-2 ratio {r[np.isin(kind, RANK2)].max():.3f} (bound {C_ORACLE}), "
              f"par_b landmarks where it picks rank 2: {int((r[kind == 'par_b'] > C_BASIC).sum())}")
        assert r[np.isin(kind, RANK2)].max() <= C_ORACLE
        assert r[np.isin(kind, ("one", "par_a", "twice_same"))].max() <= C_BASIC
        assert np.all(r[kind == "none"] == 0.0)


@pytest.fixture(scope="module")
def triangulated(world):
    """The landmarks of both precisions at both states: [precision][state] -> (poses read back, xy).
    State 0 comes from bos_create (landmark_xy = NULL), state 1 from bos_set_state + bos_triangulate on
    the running handle."""
    P, kinds, states = world
    out = {}
    for precision in (bos.BOS_FP64, bos.BOS_FP32):
        S = bos.Solver(P, precision=precision, triangulate=True)
        res = [S.get_state()]
        S.set_state(states[1][0], np.full((P.NL, 2), 7.0))   # the landmarks are to be overwritten, M = 0 too
        before, _ = S.get_state()
        S.triangulate()
        after, lm = S.get_state()
        assert np.array_equal(before, after)                  # poses untouched, bit for bit
        res.append((after, lm))
        S.close()
        out[precision] = res
    return out


@pytest.mark.parametrize("state", [0, 1])
@pytest.mark.parametrize("precision", [bos.BOS_FP64, bos.BOS_FP32])
def test_cases_against_mp(world, triangulated, precision, state):
    P, kinds, states = world
    pose, ref = states[state]
    got_pose, xy = triangulated[precision][state]
    assert np.array_equal(got_pose, pose)   # the reference's inputs are the handle's, bit for bit
    _check(xy, kinds, ref, C_DEVICE, f"precision {precision} state {state}")


@pytest.mark.parametrize("state", [0, 1])
def test_fp32_handle_same_landmarks(triangulated, state):
    """The kernel computes in double whatever the handle's precision: the same bits."""
    assert np.array_equal(triangulated[bos.BOS_FP64][state][1], triangulated[bos.BOS_FP32][state][1])


@pytest.mark.parametrize("precision", [bos.BOS_FP64, bos.BOS_FP32])
def test_landmark_cache_after_triangulate(precision):
    """bos_triangulate on a running handle writes the landmark cache the J+H build reads (a plain cast
    of the fp64 landmarks): the next linearization equals, bit for bit, that of a fresh handle created
    with those landmarks (whose caches the host uploads; the pose caches are the host's in both)."""
    P = bos.synthetic(200, 300, 8, seed=5)
    moved = P.pose_xyt + np.random.default_rng(8).normal(0, 0.02, P.pose_xyt.shape)
    moved[P.fixed] = P.pose_xyt[P.fixed]
    S = bos.Solver(P, precision=precision)
    S.set_state(moved, P.lm_xy)
    S.triangulate()
    pose, lm = S.get_state()
    assert np.array_equal(pose, moved)
    assert np.abs(lm - P.lm_xy).max() > 1e-3     # not the landmarks the handle's cache held before
    st = S.linearize()
    sys_a = S.export_system()
    S.close()
    F = bos.Solver(bos.Problem(moved, lm, P.b_pose, P.b_lm, P.b_z, P.o_src, P.o_dst, P.o_z, P.o_omega, P.fixed),
                   precision=precision)
    st_f = F.linearize()
    sys_f = F.export_system()
    F.close()
    assert np.abs(sys_a[2]).max() > 1.0 and np.abs(sys_a[3]).max() > 0.0
    for a, b in zip(sys_a, sys_f):
        assert np.array_equal(a, b)
    assert st["chi2"] == st_f["chi2"] and st["n_robust"] == st_f["n_robust"]
