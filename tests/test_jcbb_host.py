"""JCBB on the host: bos_plan_mf_jcbb (the frames' all-pairings hypotheses through bos_plan_mf_joint_compatibility's
code, then the serial search of csrc/host/jcbb.hpp) and bos_jcbb_search_host (the search alone on a given S and e)
against the enumeration of tests/jcbb_ref.py, on the systems of test_node_cov_host.py.

The spurious frame's two conditions (the winner has fewer pairings than the bearings with an individually
admissible candidate; a node is cut by a gate at depth >= 2) are asserted first, from the enumeration on the host
twin's S, wherever the world has a pair of one pose's landmarks with |rho| > jcbb_ref.SPURIOUS_RHO = 0.630 (the
bound below which no offset inside the single gate can fail the second gate: jcbb_ref's docstring): on C1 (0.68,
asserted to be such a world) under its three plans. The edge-case world (0.45), mini and synthetic(60, 120, 6)
(< 0.003) have no such pair; there the figures are printed, and the frame is compared with the enumeration like
every other. A hand-made S with rho = 0.95 shows the same conditions on the search alone."""
import ctypes

import numpy as np
import pytest

import bos
import jcbb_ref as R
from joint_ref import ldl_prefix
from test_node_cov_host import _case

SCHUR, SUPERNODAL = bos.BOS_SOLVER_SCHUR, bos.BOS_SOLVER_SUPERNODAL
PLANS = [("mini", SCHUR, 0), ("c1", SCHUR, 0), ("c1", SUPERNODAL, 0), ("c1", SCHUR, 40), ("edge_cases", SCHUR, 0)]
_cache = {}


def _world(which, solver, leaf=0):
    key = (which, solver, leaf)
    if key not in _cache:
        P, Hl, _ = _case(which)
        info = bos.plan_inspect(P, 0, 1, entries=True, solver=solver, schur_leaf=leaf)
        vals = np.asarray(Hl[info["rows"], info["cols"]]).ravel()
        kw = dict(solver=solver, schur_leaf=leaf)

        def run(frames, batch=0, max_nodes=0):
            return bos.plan_mf_jcbb(P, vals, frames, R.GATES, max_nodes=max_nodes, max_batch=batch, **kw)

        def assoc(pose, z, om, k):
            o = bos.plan_mf_associate_bearings(P, vals, pose, z, om, gate=R.GATES[0], k=k, **kw)
            return o["cand_landmark"], o["cand_var"]

        def system(frame):
            o = run([frame])
            return o["innovation_cov"][0], o["innovation"]

        def joint(hyps):
            return bos.plan_mf_joint_compatibility(P, vals, hyps, **kw)

        def systems(frames):
            o = run(frames)
            return [(o["innovation_cov"][f], o["innovation"][R.frame_slices(o, f)[1]]) for f in range(len(frames))]

        F = R.make_frames(P, (P.pose_xyt, P.lm_xy), assoc, system, systems)
        _cache[key] = (P, vals, F, run, joint, run(R.frame_list(F)))
    return _cache[key]


def _unbounded(cands, S, e):
    """The search with the bound off where that is feasible, else with the largest budget"""
    if R.leaves(cands) <= 1 << 20:
        return bos.jcbb_search_host(cands, S, e, R.GATES, max_nodes=1 << 26, no_bound=True)
    return bos.jcbb_search_host(cands, S, e, R.GATES, max_nodes=1 << 26)


@pytest.mark.parametrize("which,solver,leaf", PLANS)
def test_frames_equal_the_enumeration(which, solver, leaf):
    """Every frame of at most 4096 leaves: assignment, count, NIS and prefix bits of the enumeration; full and deep:
    those of the search without the bound (deep: 7.6e8 leaves, with the largest budget). The named frames do what
    their names say."""
    P, _, F, _, _, out = _world(which, solver, leaf)
    f = R.NAMES.index("spurious")
    _, p = R.frame_slices(out, f)
    holds = R.spurious_holds(F["spurious"][3], out["innovation_cov"][f], out["innovation"][p])
    print(f"  {which} spurious: |rho| {F['spurious/rho']:.3f} (needed {R.SPURIOUS_RHO:.3f}); holds, paired, individually admissible, "
          f"gate cuts at depth >= 2: {holds}")
    assert F["spurious/rho"] > R.SPURIOUS_RHO or which != "c1"
    if F["spurious/rho"] > R.SPURIOUS_RHO:
        assert holds[0] and holds[1] < holds[2] and holds[3] >= 1
    skipped = []
    for f, name in enumerate(R.NAMES):
        cands = F[name][3]
        big = R.leaves(cands) > R.BRUTE_LEAVES
        ref = R.check_frame(out, f, cands, _unbounded if big else None, f"{which} {name}")
        b, _ = R.frame_slices(out, f)
        print(f"  {which} {name}: m {len(cands)} P {sum(map(len, cands))} leaves {R.leaves(cands)} paired {out['n_paired'][f]} "
              f"nis {out['joint_nis'][f]:.4g} nodes {out['nodes'][f]} runner-up {ref['runner_up'] if ref else None}")
        if big:
            skipped.append(name)
    assert set(skipped) <= {"full", "deep"}
    n = lambda name: out["n_paired"][R.NAMES.index(name)]
    m = lambda name: len(F[name][3])
    assert n("clean") == m("clean") and n("full") == m("full") and n("deep") == m("deep")
    c = F["conflict"][3]
    assert c[0][0] == c[1][0] and n("conflict") == m("conflict")
    b, _ = R.frame_slices(out, R.NAMES.index("twin"))
    assert list(out["assignment"][b]) == [F["twin"][3][0][0], -1]
    assert n("no_candidates") == m("no_candidates") - 2 and n("empty") == 0
    b, _ = R.frame_slices(out, R.NAMES.index("no_candidates"))
    assert out["assignment"][b][1] == -1 and out["assignment"][b][-1] == -1
    assert np.all(F["fixed_pose"][0] == P.fixed) and len(set(F["two_poses"][0].tolist())) == 2



@pytest.mark.parametrize("which,solver,leaf", PLANS)
def test_builders_meet_the_skip_cap(which, solver, leaf):
    """What tests/test_gpu_jcbb.py compares between the GPU and the host twin: at most one named frame per world (twin,
    an exact tie by construction) is closer to its runner-up than joint_ref's NIS bound, here on the host twin's own S
    with tol = min(sparse tol, TOL_CAP)."""
    from marginals_ref import TOL_CAP, sparse_tol
    P, vals, F, _, _, out = _world(which, solver, leaf)
    tol, _ = sparse_tol(P, _case(which)[1])
    close = R.close_frames(P, vals, F, R.NAMES, out, min(tol, TOL_CAP), solver=solver, schur_leaf=leaf)
    print(f"  {which} solver {solver} leaf {leaf}: closer than the bound: {close}")
    assert len(close) <= 1


def test_twin_is_an_exact_tie():
    """(X, nothing) and (nothing, X) have the same NIS bits: the lexicographic rule decides."""
    _, _, F, run, _, _ = _world("c1", SCHUR)
    out = run([F["twin"]])
    S, e = out["innovation_cov"][0], out["innovation"]
    assert S[0, 0] == S[1, 1] and e[0] == e[1]
    ref = R.brute_force(F["twin"][3], S, e)
    assert ref["runner_up"] == (1, ref["joint_nis"]) and ref["choice"] == (0, R.NOTHING)


@pytest.mark.parametrize("which,solver,leaf", PLANS)
def test_against_the_joint_twin(which, solver, leaf):
    """joint_nis and prefix_nis are plan_mf_joint_compatibility's of the winning hypothesis, innovation and
    innovation_cov those of the all-pairings hypothesis, bit for bit."""
    _, _, F, _, joint, out = _world(which, solver, leaf)
    R.check_against_joint(out, R.frame_list(F), joint)


@pytest.mark.parametrize("which,solver,leaf", [("mini", SCHUR, 0), ("c1", SCHUR, 0), ("c1", SCHUR, 40), ("edge_cases", SCHUR, 0)])
def test_exact_rules(which, solver, leaf):
    """Two calls, the repeated frame, order, company and one frame per batch: identical bits."""
    _, _, F, run, _, _ = _world(which, solver, leaf)
    R.check_exact_rules(R.frame_list(F), run)


def _admissible(frame, out, f):
    """The returned hypothesis, re-checked through ldl_prefix on the frame's own S_all and e_all"""
    b, p = R.frame_slices(out, f)
    cands = frame[3]
    start = np.concatenate([[0], np.cumsum([len(c) for c in cands])]).astype(int)
    asg = out["assignment"][b]
    q = [start[t] + cands[t].index(int(l)) for t, l in enumerate(asg) if l >= 0]
    assert len(set(asg[asg >= 0].tolist())) == len(q) == out["n_paired"][f]
    pre = ldl_prefix(out["innovation_cov"][f][np.ix_(q, q)], out["innovation"][p][q]) if q else np.zeros(0)
    assert np.all(np.isfinite(pre)) and np.all(pre <= R.GATES[:len(pre)])
    assert out["joint_nis"][f] == (pre[-1] if q else 0.0)


@pytest.mark.parametrize("budget", [1, 50])
def test_budget(budget):
    """With max_nodes 1 and 50 the frames that need more do not finish (moved needs 180): complete == 0, an
    admissible hypothesis; the others are the full search's."""
    _, _, F, run, _, _ = _world("c1", SCHUR)
    names = R.NAMES + ("moved",)
    frames = [F[n] for n in names]
    full = run(frames)
    out = run(frames, max_nodes=budget)
    assert np.all(out["nodes"] <= budget) and full["nodes"][-1] > 50
    for f, name in enumerate(names):
        _admissible(frames[f], out, f)
        if full["nodes"][f] > budget:
            assert out["complete"][f] == 0 and out["nodes"][f] == budget, name
        else:
            assert out["complete"][f] == 1, name
            R.same_frame(full, f, out, f)


def _raw(frame_start, pose, z, omega, cand_start, cand_landmark):
    return {"frame_start": frame_start, "pose": pose, "z": z, "omega": omega, "cand_start": cand_start, "cand_landmark": cand_landmark}


def bad_calls(NP, NL):
    """name -> (raw frames, gate, max_nodes) of every BOS_ERR_INVALID case"""
    g = R.GATES
    big_m, big_p = bos.JCBB_MAX_BEARINGS + 1, bos.JOINT_MAX_M + 1
    ok = lambda **kw: {**_raw([0, 2], [1, 1], [0.1, 0.2], None, [0, 1, 2], [0, 1]), **kw}
    gate = lambda j, v: np.concatenate([g[:j], [v], g[j + 1:]])
    return {"frame_start_not_zero": (ok(frame_start=[1, 2]), g, 0),
            "frame_start_decreasing": (_raw([0, 2, 1], [1], [0.1], None, [0, 1], [0]), g, 0),
            "cand_start_not_zero": (ok(cand_start=[1, 1, 2]), g, 0),
            "cand_start_decreasing": (ok(cand_start=[0, 2, 1], cand_landmark=[0]), g, 0),
            "too_many_bearings": (_raw([0, big_m], [1] * big_m, [0.1] * big_m, None, [0] * (big_m + 1), []), g, 0),
            "too_many_pairings": (_raw([0, 2], [1, 1], [0.1, 0.2], None, [0, 17, big_p], list(range(17)) + list(range(16))), g, 0),
            "pose_low": (ok(pose=[-1, 1]), g, 0), "pose_high": (ok(pose=[1, NP]), g, 0),
            "landmark_low": (ok(cand_landmark=[0, -2]), g, 0), "landmark_high": (ok(cand_landmark=[NL, 1]), g, 0),
            "landmark_twice": (ok(cand_start=[0, 2, 2], cand_landmark=[3, 3]), g, 0),
            "z_nan": (ok(z=[np.nan, 0.1]), g, 0), "z_inf": (ok(z=[0.1, np.inf]), g, 0),
            "omega_zero": (ok(omega=[1.0, 0.0]), g, 0), "omega_negative": (ok(omega=[-1.0, 1.0]), g, 0),
            "omega_nan": (ok(omega=[np.nan, 1.0]), g, 0), "omega_inf": (ok(omega=[1.0, np.inf]), g, 0),
            "gate_nan": (ok(), gate(3, np.nan), 0), "gate_zero": (ok(), gate(0, 0.0), 0), "gate_negative": (ok(), gate(31, -1.0), 0),
            "max_nodes_negative": (ok(), g, -1)}


def test_argument_errors_leave_the_outputs():
    P, vals, _, _, _, _ = _world("mini", SCHUR)
    cs, opt = P.c_struct(), bos.options(SCHUR)
    v = np.ascontiguousarray(vals)
    dp, ip, lp = ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(ctypes.c_int64)
    for name, (raw, gate, max_nodes) in bad_calls(P.NP, P.NL).items():
        a = {k: (None if x is None else np.ascontiguousarray(x, dtype=np.float64 if k in ("z", "omega") else np.int32)) for k, x in raw.items()}
        gate = np.ascontiguousarray(gate, dtype=np.float64)
        ints = [np.full(64, 7, dtype=np.int32) for _ in range(3)]
        dbl = [np.full(64, 7.0) for _ in range(3)] + [np.full(2048, 7.0)]
        nodes = np.full(8, 7, dtype=np.int64)
        ptr = lambda x, t: None if x is None else x.ctypes.data_as(t)
        rc = bos.lib().bos_plan_mf_jcbb(ctypes.byref(cs), ctypes.byref(opt), ptr(v, dp), len(a["frame_start"]) - 1, ptr(a["frame_start"], ip),
                                        ptr(a["pose"], ip), ptr(a["z"], dp), ptr(a["omega"], dp), ptr(a["cand_start"], ip),
                                        ptr(a["cand_landmark"], ip), ptr(gate, dp), max_nodes, 0, ptr(ints[0], ip), ptr(ints[1], ip),
                                        ptr(dbl[0], dp), ptr(dbl[1], dp), ptr(ints[2], ip), ptr(dbl[2], dp), ptr(dbl[3], dp), ptr(nodes, lp))
        assert rc == -1, name
        assert all(np.all(o == 7) for o in ints + dbl + [nodes]), name
    # ends that do not agree: the library has no lengths, the binding refuses them
    for raw in (_raw([0, 3], [1, 1], [0.1, 0.2], None, [0, 1, 2], [0, 1]), _raw([0, 2], [1, 1], [0.1, 0.2], None, [0, 1, 3], [0, 1]),
                _raw([0, 1], [1, 1], [0.1, 0.2], None, [0, 1, 2], [0, 1]), _raw([0, 2], [1, 1], [0.1, 0.2], None, [0, 1, 1], [0, 1])):
        with pytest.raises(bos.BosError, match="do not agree"):
            bos.plan_mf_jcbb(P, vals, raw, R.GATES)
    out = bos.plan_mf_jcbb(P, vals, [], R.GATES)
    assert len(out["n_paired"]) == 0 and out["innovation_cov"] == []
    # +inf gates are allowed; the list form with -1 padding is the list form without
    inf = np.full(bos.JOINT_MAX_M, np.inf)
    x = bos.plan_mf_jcbb(P, vals, [([1, 1], [0.1, 0.2], None, np.array([[0, 1, -1], [1, -1, -1]]))], inf)
    y = bos.plan_mf_jcbb(P, vals, [(1, [0.1, 0.2], [1.0, 1.0], [[0, 1], [1]])], inf)
    assert x["n_paired"][0] == 2 and np.array_equal(x["assignment"], y["assignment"]) and x["joint_nis"][0] == y["joint_nis"][0]


# ---- bos_jcbb_search_host on hand-made systems ----------------------------------------------------------
def test_diagonal_tie_is_lexicographic():
    """Diagonal S with equal entries and equal e: every pairing costs the same, so among the hypotheses of two
    pairings the smallest choice vector wins: (position 0, position 0) where the lists allow it."""
    cands = [[5, 6], [7, 5]]
    S, e = 2.0 * np.eye(4), np.full(4, 0.5)
    out = bos.jcbb_search_host(cands, S, e, R.GATES)
    ref = R.brute_force(cands, S, e)
    assert list(out["assignment"]) == [5, 7] == list(ref["assignment"]) and out["joint_nis"] == ref["joint_nis"] == 0.25
    assert ref["runner_up"] == (2, 0.25)
    cands = [[5, 6], [5, 7]]                                     # (0, 0) uses landmark 5 twice: (0, 1) is next
    out = bos.jcbb_search_host(cands, S, e, R.GATES)
    assert list(out["assignment"]) == [5, 7] == list(R.brute_force(cands, S, e)["assignment"])
    out = bos.jcbb_search_host([[5], [5]], 2.0 * np.eye(2), np.full(2, 0.5), R.GATES)
    assert list(out["assignment"]) == [5, -1] and out["n_paired"] == 1 and list(out["prefix_nis"]) == [0.125, 0.125]


def test_bad_pivot_cuts_the_subtree():
    """Pairings 0 and 1 together give D_1 = 0: the pair is never chosen, whatever it would score."""
    S = np.array([[2.0, 1.0, 0.0], [1.0, 0.5, 0.0], [0.0, 0.0, 1.0]])
    e = np.array([0.1, 0.1, 0.1])
    cands = [[1], [2], [3]]
    inf = np.full(bos.JOINT_MAX_M, np.inf)
    out = bos.jcbb_search_host(cands, S, e, inf)
    ref = R.brute_force(cands, S, e, inf)
    assert out["n_paired"] == ref["n_paired"] == 2 and np.array_equal(out["assignment"], ref["assignment"])
    assert out["joint_nis"] == ref["joint_nis"] and np.isfinite(out["joint_nis"])
    neg = bos.jcbb_search_host([[1]], np.array([[-1.0]]), np.array([0.1]), inf)
    assert neg["n_paired"] == 0 and neg["joint_nis"] == 0.0 and neg["complete"] == 1


def test_infinite_gates_and_the_bound():
    """+inf gates: everything with good pivots is admissible; the search with and without the bound and the
    enumeration agree on random SPD systems, and the bound saves nodes."""
    rng = np.random.default_rng(5)
    inf = np.full(bos.JOINT_MAX_M, np.inf)
    saved = 0
    for trial in range(20):
        cands = [[int(x) for x in rng.choice(6, rng.integers(0, 4), replace=False)] for _ in range(rng.integers(1, 6))]
        n = sum(map(len, cands))
        A = rng.normal(size=(n, n + 2))
        S, e = A @ A.T + 0.1 * np.eye(n), rng.normal(size=n)
        for gate in (inf, R.GATES):
            ref = R.brute_force(cands, S, e, gate)
            a = bos.jcbb_search_host(cands, S, e, gate)
            b = bos.jcbb_search_host(cands, S, e, gate, no_bound=True)
            for o in (a, b):
                assert np.array_equal(o["assignment"], ref["assignment"]) and o["joint_nis"] == ref["joint_nis"], trial
                assert np.array_equal(o["prefix_nis"], ref["prefix_nis"]) and o["complete"] == 1
            assert a["nodes"] <= b["nodes"]
            saved += b["nodes"] - a["nodes"]
    assert saved > 0


def test_spurious_on_a_correlated_system():
    """Three bearings with one candidate each, innovations correlated with rho = 0.95, the second moved by 1.8
    standard deviations: inside its own gate (3.24 <= 3.84), rejected with the first (prefix 2 is 33 > 5.99): the
    winner has two pairings where three bearings have an individually admissible candidate, and a node is cut by
    a gate at depth 2."""
    rho = 0.95
    S = np.full((3, 3), rho) + (1 - rho) * np.eye(3)
    e = np.array([0.01, 1.8, -0.01])
    cands = [[1], [2], [3]]
    holds, paired, alone, deep = R.spurious_holds(cands, S, e)
    print(f"spurious on rho {rho}: paired {paired} of {alone} individually admissible, {deep} hypotheses cut at depth >= 2")
    assert holds and paired == 2 and alone == 3 and deep >= 1
    out = bos.jcbb_search_host(cands, S, e, R.GATES)
    ref = R.brute_force(cands, S, e)
    assert list(out["assignment"]) == [1, -1, 3] == list(ref["assignment"]) and out["joint_nis"] == ref["joint_nis"]


def test_deep_needs_the_count_bound():
    """deep is quick with the bound (a few dozen nodes) and does not finish in 2^16 nodes without it."""
    _, _, F, _, _, out = _world("c1", SCHUR)
    f = R.NAMES.index("deep")
    _, p = R.frame_slices(out, f)
    assert out["nodes"][f] < 1000
    slow = bos.jcbb_search_host(F["deep"][3], out["innovation_cov"][f], out["innovation"][p], R.GATES, max_nodes=1 << 16, no_bound=True)
    assert slow["complete"] == 0 and slow["nodes"] == 1 << 16
