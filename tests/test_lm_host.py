"""CPU tests of the Levenberg-Marquardt feature: the step-control rule the device, the CPU twin and
these tests share (bos_lm_rule_apply) against a Python twin on a table of cases, and the CPU twin
(CpuGN.cost / CpuGN.optimize) against the oracle reference of tests/lm_ref.py."""
import math

import numpy as np
import pytest

import bos
import lm_ref as R
from conftest import C1
from helpers import knife_edge_bearings, to_oracle

INF, NAN = float("inf"), float("nan")


def _state(lam=1e-2, nu=2.0, cost=100.0, iteration=0, accepted=0, rejected=0, done=0, reason=0):
    return {"lambda": lam, "nu": nu, "cost": cost, "iteration": iteration, "accepted": accepted, "rejected": rejected,
            "done": done, "reason": reason}


# (name, state, options, cost_trial, predicted, max_dx, solver_info, expected accepted, expected reason)
RULE_CASES = [
    ("accept, small gain: lambda grows", _state(), {}, 99.0, 10.0, 0.5, 0, 1, 0),
    ("accept, gain 1/2: lambda kept", _state(), {}, 95.0, 10.0, 0.5, 0, 1, 0),
    ("accept, large gain: factor 1/3", _state(), {}, 90.0, 10.0, 0.5, 0, 1, 0),
    ("accept, gain > 1", _state(), {}, 80.0, 10.0, 0.5, 0, 1, 0),
    ("accept resets nu", _state(nu=16.0), {}, 90.0, 10.0, 0.5, 0, 1, 0),
    ("reject: cost up", _state(), {}, 101.0, 10.0, 0.5, 0, 0, 0),
    ("reject: cost equal", _state(), {}, 100.0, 10.0, 0.5, 0, 0, 0),
    ("reject doubles nu again", _state(nu=8.0, rejected=2, iteration=2), {}, 150.0, 10.0, 0.5, 0, 0, 0),
    ("reject: info != 0 although the cost fell", _state(), {}, 50.0, 10.0, 0.5, 3, 0, 0),
    ("reject: NaN trial cost", _state(), {}, NAN, 10.0, 0.5, 0, 0, 0),
    ("reject: infinite trial cost", _state(), {}, INF, 10.0, 0.5, 0, 0, 0),
    ("reject: predicted zero", _state(), {}, 50.0, 0.0, 0.5, 0, 0, 0),
    ("reject: predicted negative", _state(), {}, 50.0, -1.0, 0.5, 0, 0, 0),
    ("reject: predicted NaN", _state(), {}, 50.0, NAN, 0.5, 0, 0, 0),
    ("clamp at lambda_min", _state(lam=2e-12), {}, 90.0, 10.0, 0.5, 0, 1, 0),
    ("clamp at lambda_max", _state(lam=9e11, nu=4.0), {}, 101.0, 10.0, 0.5, 0, 0, 0),
    ("stop 1 on an accepted step", _state(), {}, 99.999, 1e-3, 1e-7, 0, 1, 1),
    ("stop 1 on a rejected step", _state(), {}, 100.5, 1e-3, 1e-7, 0, 0, 1),
    ("stop 1 before stop 2", _state(), {"f_tol": 1e-3}, 99.9999, 1e-3, 1e-7, 0, 1, 1),
    ("stop 1 disabled", _state(), {"dx_tol": 0.0}, 99.0, 10.0, 0.0, 0, 1, 0),
    ("max |dx| NaN is no convergence", _state(), {}, NAN, NAN, NAN, 0, 0, 0),
    ("stop 2", _state(), {"f_tol": 1e-3}, 99.95, 0.1, 0.5, 0, 1, 2),
    ("stop 2 disabled", _state(), {"f_tol": 0.0}, 100.0 - 1e-12, 1e-11, 0.5, 0, 1, 0),
    ("stop 2 needs an accepted step", _state(), {"f_tol": 1e-3}, 100.01, 0.1, 0.5, 0, 0, 0),
    ("stop 4: rejected at lambda_max", _state(lam=1e12), {}, 101.0, 10.0, 0.5, 0, 0, 4),
    ("no stop 4 when lambda only reaches lambda_max now", _state(lam=6e11), {}, 101.0, 10.0, 0.5, 0, 0, 0),
    ("no stop 4 on an accepted step at lambda_max", _state(lam=1e12), {}, 99.0, 10.0, 0.5, 0, 1, 0),
    ("stop 4 before stop 3", _state(lam=1e12, iteration=49), {}, 101.0, 10.0, 0.5, 0, 0, 4),
    ("stop 3", _state(iteration=49, accepted=40, rejected=9), {}, 99.0, 10.0, 0.5, 0, 1, 3),
    ("stop 3 on a rejected step", _state(iteration=4), {"max_iterations": 5}, 101.0, 10.0, 0.5, 0, 0, 3),
    ("frozen after done", _state(done=1, reason=1, iteration=7, accepted=5, rejected=2), {}, 50.0, 10.0, 0.5, 0, 0, 1),
]


@pytest.mark.parametrize("case", RULE_CASES, ids=[c[0] for c in RULE_CASES])
def test_rule_matches_python_twin(case):
    _, st, okw, Ft, pred, mdx, info, want_acc, want_reason = case
    o = R.options(**okw)
    got_st, got_rec, got_counted = bos.lm_rule_apply(st, bos.lm_options(**okw), Ft, pred, mdx, info)
    ref_st, ref_rec, ref_counted = R.rule(st, o, Ft, pred, mdx, info)
    assert got_counted == ref_counted == (not st["done"])
    assert got_rec["accepted"] == ref_rec["accepted"] == want_acc
    assert got_st["reason"] == ref_st["reason"] == want_reason
    for k in ("iteration", "accepted", "rejected", "done"):
        assert got_st[k] == ref_st[k], k
    for k in ("lambda", "nu", "cost"):
        assert got_st[k] == ref_st[k], (k, got_st[k], ref_st[k])
    assert o["lambda_min"] <= got_st["lambda"] <= o["lambda_max"]
    if not got_counted:   # frozen: nothing moved
        assert got_st == st
        return
    for k, v in ref_rec.items():
        assert got_rec[k] == v or (isinstance(v, float) and math.isnan(v) and math.isnan(got_rec[k])), (k, got_rec[k], v)


def test_rule_sequences():
    """nu doubles over consecutive rejections (lambda x 2, 4, 8), an acceptance resets it."""
    o, lo = R.options(), bos.lm_options()
    st = _state(lam=1e-4)
    lams = []
    for Ft in (101.0, 102.0, 103.0):
        st, rec, _ = bos.lm_rule_apply(st, lo, Ft, 10.0, 0.5, 0)
        lams.append(st["lambda"])
    assert lams == [2e-4, 8e-4, 64e-4] and st["nu"] == 16.0 and st["rejected"] == 3
    st, rec, _ = bos.lm_rule_apply(st, lo, 95.0, 10.0, 0.5, 0)
    assert rec["accepted"] == 1 and st["nu"] == 2.0 and st["cost"] == 95.0 and st["lambda"] == 64e-4
    assert R.rule(_state(lam=64e-4, nu=16.0, rejected=3, iteration=3), o, 95.0, 10.0, 0.5, 0)[0] == st


def test_default_options():
    o = bos.lm_options()
    assert {k: getattr(o, k) for k, _ in o._fields_} == R.DEFAULTS


@pytest.fixture(scope="module")
def c1():
    return bos.load_g2o(C1)


@pytest.fixture(scope="module")
def inputs(c1):
    """name -> (bos problem, oracle problem)"""
    pert = R.with_poses(c1, R.perturbed_poses(c1))
    return {"plain": (c1, to_oracle(c1)), "perturbed": (pert, to_oracle(pert))}


@pytest.mark.parametrize("which", ["plain", "perturbed"])
def test_cpu_cost(inputs, which):
    P, Q = inputs[which]
    C = bos.CpuGN(P, threads=2)
    pose, lm = C.get_state()
    for kt in (1.0, 1e30, 1e-3):
        C.set_kernel_threshold(kt)
        got = C.cost()
        F, chi, nrob = R.cost(Q, pose, lm, kt)
        print(f"cpu cost {which} kt {kt:g}: F {got['cost']:.12g} ref {F:.12g} chi2 {got['chi2']:.12g} robust {nrob}")
        assert abs(got["cost"] - F) <= 1e-9 * F
        assert abs(got["chi2"] - chi) <= 1e-9 * chi
        assert got["n_robust"] == nrob
        if kt == 1e30:
            assert got["cost"] == got["chi2"] and nrob == 0
    C.close()


def test_cpu_cost_is_the_step_chi2(c1):
    """With the threshold past every rho, F is the chi2 the GN step reports."""
    C = bos.CpuGN(c1, threads=2)
    C.set_kernel_threshold(1e30)
    F = C.cost()["cost"]
    chi = C.step()
    C.close()
    assert abs(F - chi) <= 1e-9 * chi


def test_cpu_one_step_parity_perturbed(inputs):
    """Fourteen single iterations of the CPU twin on "perturbed" (kt 1e30, lambda0 1e-4), each against
    one reference iteration from the twin's own previous state and lambda."""
    P, Q = inputs["perturbed"]
    kt = 1e30
    C = bos.CpuGN(P, threads=2)
    C.set_kernel_threshold(kt)
    o = R.options(max_iterations=1, dx_tol=0.0, f_tol=0.0)
    lam, nu, flags, worst = 1e-4, 2.0, [], {}
    for i in range(14):
        before = C.get_state()
        Qs = to_oracle(R.with_poses(P, before[0]))
        Qs.lm_xy = before[1].copy()
        assert len(knife_edge_bearings(Qs)[0]) == 0
        got = C.optimize(lambda0=1e-4 if i == 0 else 0.0, max_iterations=1, dx_tol=0.0, f_tol=0.0)
        after = C.get_state()
        assert got["iterations"] == 1 and got["reason"] == 3 and len(got["trace"]) == 1
        rec = {k: got["trace"][0][k].item() for k in got["trace"].dtype.names}
        st = R.new_state(lam, R.cost(Q, before[0], before[1], kt)[0], nu)
        it = R.iterate(Q, before[0], before[1], kt, st, o)
        R.assert_comparable(it)
        for k, v in R.check_iteration(f"cpu twin it {i}", rec, before, after, got["lambda_final"], it).items():
            worst[k] = max(worst.get(k, 0.0), v)
        assert got["cost_final"] == (rec["cost_trial"] if rec["accepted"] else rec["cost"])
        flags.append(rec["accepted"])
        lam, nu = it.st["lambda"], it.st["nu"]
        lam = got["lambda_final"]
    C.close()
    print("cpu twin worst err/tol:", {k: f"{v:.3g}" for k, v in worst.items()}, "flags", flags)
    assert flags.count(0) >= 2 and flags.count(1) >= 5


def test_cpu_optimize_converges_on_plain(inputs):
    P, Q = inputs["plain"]
    C = bos.CpuGN(P, threads=2)
    got = C.optimize(lambda0=0.01, dx_tol=1e-4)
    _, _, st, its = R.run(Q, Q.pose_xyt, Q.lm_xy, 1.0, R.options(lambda0=0.01, dx_tol=1e-4))
    C.close()
    print(f"cpu twin plain: {got['iterations']} iterations (ref {st['iteration']}), cost {got['cost_final']:.10g} "
          f"(ref {st['cost']:.10g}), lambda {got['lambda_final']:.3g}")
    assert got["reason"] == st["reason"] == 1
    assert got["iterations"] <= st["iteration"] + 2 < 50
    assert abs(got["cost_final"] - st["cost"]) <= 1e-6 * st["cost"]
    assert np.all(np.diff(got["trace"]["cost"]) <= 0.0)
    assert got["accepted"] + got["rejected"] == got["iterations"]
