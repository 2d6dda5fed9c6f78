"""CPU tests of the prior factors (bos_set_priors): the shared arithmetic (bos.prior_terms, csrc/host/prior.hpp)
against its NumPy transcription bit for bit, and the CPU twin (CpuGN.set_priors) against the oracle
reference of tests/prior_ref.py."""
import numpy as np
import pytest

import bos
import oracle as O
import prior_ref as R
from conftest import C1, MINI
from helpers import close_state, literal_oracle, to_oracle


def _same_bits(got, ref, what):
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    assert got.tobytes() == ref.tobytes(), (what, got, ref)


def _check_terms(kind, state, mean, omega):
    A, g, rho = bos.prior_terms(kind, state, mean, omega)
    Ar, gr, rhor, _ = (R.pose_terms if kind == "pose" else R.landmark_terms)(state, mean, omega)
    _same_bits(A, Ar, (kind, "A"))
    _same_bits(g, gr, (kind, "g"))
    _same_bits([rho], [rhor], (kind, "rho"))
    return A, g, rho


def _rand_sym(rng, d, scale):
    M = rng.normal(size=(d, d)) * scale
    return 0.5 * (M + M.T)


@pytest.mark.parametrize("kind", ["pose", "landmark"])
def test_prior_terms_random_bit_for_bit(kind):
    rng = np.random.default_rng(20 if kind == "pose" else 21)
    d = 3 if kind == "pose" else 2
    for i in range(200):
        scale = 10.0 ** rng.integers(-3, 4)
        state = rng.normal(size=d) * scale
        mean = state + rng.normal(size=d) * 10.0 ** rng.integers(-6, 1)
        if kind == "pose":   # angles anywhere in a few turns: the wrap runs on many of them
            state[2] = rng.uniform(-np.pi, np.pi)
            mean[2] = rng.uniform(-7.0, 7.0)
        _check_terms(kind, state, mean, _rand_sym(rng, d, 10.0 ** rng.integers(-2, 5)))


def test_prior_terms_wrap():
    """theta - m2 = 2 pi - 0.1: the error's angle is -0.1, not 6.18."""
    th, m2 = 3.0, 3.0 - (2 * np.pi - 0.1)
    om = np.diag([0.0, 0.0, 2.0])
    A, g, rho = _check_terms("pose", [1.0, 2.0, th], [1.0, 2.0, m2], om)
    e2 = R.pose_terms([1.0, 2.0, th], [1.0, 2.0, m2], om)[3][2]
    assert abs(e2 - (-0.1)) <= 4 * np.finfo(float).eps * 2 * np.pi
    assert abs(g[2] - 2.0 * -0.1) <= 1e-14 and abs(rho - 2.0 * 0.01) <= 1e-14


def test_prior_terms_semidefinite():
    """Heading only and position only."""
    A, g, rho = _check_terms("pose", [3.0, -4.0, 0.5], [2.5, -4.5, 0.25], np.diag([0.0, 0.0, 100.0]))
    assert np.array_equal(A, [0.0, 0.0, 0.0, 0.0, 0.0, 100.0]) and np.array_equal(g[:2], [0.0, 0.0]) and rho == 100.0 * 0.0625
    A, g, rho = _check_terms("pose", [3.0, -4.0, 0.5], [2.5, -4.5, 0.25], np.diag([4.0, 4.0, 0.0]))
    # J^T Omega J with J = [[1, 0, -y], [0, 1, x], [0, 0, 1]], y = -4, x = 3
    assert np.array_equal(A, [4.0, 0.0, 4.0, 16.0, 12.0, 100.0]) and rho == 2.0
    A, g, rho = _check_terms("landmark", [1.0, 1.0], [0.0, 3.0], [[1.0, 0.0], [0.0, 0.0]])
    assert np.array_equal(A, [1.0, 0.0, 0.0]) and np.array_equal(g, [1.0, 0.0]) and rho == 1.0


def test_prior_terms_zero_omega_gives_exact_zeros():
    for kind, state, mean in (("pose", [3.1, -4.2, 0.5], [1.0, 2.0, -2.0]), ("landmark", [7.5, -1.25], [0.1, 0.2])):
        d = len(state)
        A, g, rho = _check_terms(kind, state, mean, np.zeros((d, d)))
        assert not A.any() and not g.any() and rho == 0.0


def test_prior_terms_bad_kind():
    with pytest.raises(KeyError):
        bos.prior_terms("edge", [0.0, 0.0], [0.0, 0.0], np.eye(2))
    z = np.zeros(9)
    p = bos._ptr(z, bos.ctypes.c_double)
    assert bos.lib().bos_prior_terms(2, p, p, p, p, p, p) != bos.BOS_OK


@pytest.fixture(scope="module")
def problems():
    return {"mini": bos.load_g2o(MINI), "c1": bos.load_g2o(C1)}


def _priors_for(P, name):
    if name == "mini":
        return R.random_priors(P, 1, 2, seed=5)
    return R.random_priors(P, 40, 60, seed=6)


@pytest.mark.parametrize("name", ["mini", "c1"])
def test_cpu_cost_with_priors(problems, name):
    P = problems[name]
    pri = _priors_for(P, name)
    C = bos.CpuGN(P, threads=2)
    pose, lm = C.get_state()
    base = C.cost()
    C.set_priors(**pri)
    rho = R.sum_rho(pri, P.NP, pose, lm)
    assert rho > 0.0
    for kt in (1.0, 1e30):
        C.set_kernel_threshold(kt)
        got = C.cost()
        Fr, chir, nrob = R.cost(to_oracle(P), pose, lm, kt, pri)
        print(f"cpu cost with priors {name} kt {kt:g}: F {got['cost']:.12g} ref {Fr:.12g} sum rho {rho:.6g}")
        assert abs(got["cost"] - Fr) <= 1e-9 * Fr
        assert abs(got["chi2"] - chir) <= 1e-9 * chir
        assert got["n_robust"] == nrob == (base["n_robust"] if kt == 1.0 else 0)
    C.set_kernel_threshold(1.0)
    C.set_priors()
    assert C.cost() == base
    C.close()


@pytest.mark.parametrize("name", ["mini", "c1"])
def test_cpu_steps_with_priors(problems, name):
    """Five steps of the CPU twin against the reference's: chi^2 per iteration and the final state with
    the closeness test_host.py uses between the twin and the oracle."""
    P = problems[name]
    pri = _priors_for(P, name)
    C = bos.CpuGN(P, threads=2)
    C.set_priors(**pri)
    chis = [C.step() for _ in range(5)]
    pg, lg = C.get_state()
    plain = bos.CpuGN(P, threads=2)
    plain_chi = plain.step()
    plain.close()
    C.close()
    Q = to_oracle(P)
    po, lo = Q.copy_state()
    chio = [R.step(Q, po, lo, pri)[0] for _ in range(5)]
    print(f"cpu steps with priors {name}: chi2 {chis} ref {chio}")
    assert np.allclose(chis, chio, rtol=1e-9, atol=1e-12)
    ok, ep, el = close_state(pg, lg, po, lo)
    assert ok, (ep, el)
    assert chis[0] > plain_chi   # the priors are counted


@pytest.mark.parametrize("name", ["mini", "c1"])
def test_cpu_optimize_with_priors(problems, name):
    P = problems[name]
    pri = _priors_for(P, name)
    C = bos.CpuGN(P, threads=2)
    C.set_priors(**pri)
    before = C.cost()["cost"]
    got = C.optimize(lambda0=0.01, dx_tol=1e-4)
    after = C.cost()["cost"]
    C.close()
    tr = got["trace"]
    assert got["cost_initial"] == before and got["cost_final"] == after
    assert after < before
    acc = tr[tr["accepted"] == 1]
    assert len(acc) >= 1 and np.all(acc["cost_trial"] < acc["cost"])
    assert np.all(np.diff(tr["cost"]) <= 0.0)


def test_cpu_set_priors_argument_errors(problems):
    P = problems["c1"]
    C = bos.CpuGN(P, threads=1)
    good = R.random_priors(P, 3, 3, seed=9)
    C.set_priors(**good)
    want = C.cost()
    free = [p for p in range(P.NP) if p != P.fixed]
    I3, I2 = np.eye(3), np.eye(2)
    nan, inf = float("nan"), float("inf")
    bad = [
        dict(pose=([P.NP], [[0, 0, 0]], [I3])),
        dict(pose=([-1], [[0, 0, 0]], [I3])),
        dict(landmark=([P.NL], [[0, 0]], [I2])),
        dict(landmark=([-1], [[0, 0]], [I2])),
        dict(pose=([free[0], free[0]], np.zeros((2, 3)), [I3, I3])),
        dict(landmark=([4, 7, 4], np.zeros((3, 2)), [I2, I2, I2])),
        dict(pose=([P.fixed], [[0, 0, 0]], [I3])),
        dict(pose=([free[0]], [[0, nan, 0]], [I3])),
        dict(landmark=([0], [[inf, 0]], [I2])),
        dict(pose=([free[0]], [[0, 0, 0]], [np.diag([1.0, nan, 1.0])])),
        dict(landmark=([0], [[0, 0]], [[[1.0, inf], [inf, 1.0]]])),
        dict(pose=([free[0]], [[0, 0, 0]], [[[1, 0.5, 0], [0.5 + 1e-16 + 1e-12, 1, 0], [0, 0, 1]]])),
        dict(landmark=([0], [[0, 0]], [[[1.0, 0.25], [0.26, 1.0]]])),
        dict(pose=([free[0]], [[0, 0, 0]], [np.diag([1.0, -1e-300, 1.0])])),
        dict(landmark=([0], [[0, 0]], [np.diag([-1.0, 1.0])])),
    ]
    for kw in bad:
        with pytest.raises(bos.BosError, match="bos_cpu_gn_set_priors"):
            C.set_priors(**kw)
        assert C.cost() == want, kw   # the previous set is still in force
    # allowed: semidefinite informations
    C.set_priors(pose=([free[1]], [P.pose_xyt[free[1]]], [np.diag([0.0, 0.0, 5.0])]),
                 landmark=([1], [P.lm_xy[1] + 1.0], [np.diag([1.0, 0.0])]))
    assert C.cost()["cost"] > 0.0
    C.close()
