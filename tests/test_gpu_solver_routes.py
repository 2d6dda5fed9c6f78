"""The multifrontal solve against an exact answer, kernel route by kernel route.

The solve chooses among a dozen kernel routes by front size, tree level and level population
(hip/multifrontal.hip mf_factor_t / mf_solve; the kernels are in hip/mf_*.hpp). Each case here is
one small world whose plan takes known routes (helpers.SOLVER_WORLDS; DESIGN.md §5 has the table); the routes are read from the
launch sites' own report (Solver.debug_solver_routes), and test_every_route_is_covered fails when a
route of the enum is neither taken by a case nor listed, with its reason, in UNREACHED.

Criterion (helpers.SolveReference.check): one linearize(), export_system(), step() and last_dx() at
the same state. x* is the exported system's solution refined in np.longdouble; the device's x passes
when its forward error is within 4 x, and its normwise backward error within 8 x, of the larger of two
unrefined fp64 reference solvers' on that very system (dense LAPACK Cholesky, SciPy SuperLU). The
margins cover another elimination order and MFMA / FMA summation order; a kernel that drops or
misplaces one update term lands 6+ orders of magnitude outside (tests/test_host.py proves the
criterion on the host re-run of the algorithm, and that it rejects one entry off by 1e-6).

An fp32 handle (the F32 kernel instances: the folds read the fp32 block array) exports exactly the
values its solve reads: bos_export_system expands the factored pose-landmark blocks with the same fp32
products as the fold's decode, and every other entry is the fp32 value widened, as in the solver's
fp64 copy. So the criterion applies to that handle's own export."""
import numpy as np
import pytest

import bos
from helpers import SOLVER_DAMPING, SOLVER_WORLDS, solve_reference, solver_world

pytestmark = pytest.mark.gpu

F = {n: i for i, n in enumerate(bos.Solver.FACTOR_ROUTES)}
B = {n: i for i, n in enumerate(bos.Solver.BACKWARD_ROUTES)}


def _fold_fp32(name):
    P, solver, leaf = solver_world(name)
    return bos.plan_inspect(P, solver=solver, schur_leaf=leaf)["mf_fold_fp32"]


CASES = [(n, bos.BOS_FP64) for n in sorted(SOLVER_WORLDS)] + \
        [(n, bos.BOS_FP32) for n in sorted(SOLVER_WORLDS) if _fold_fp32(n)]
IDS = [f"{n}-{'fp32' if p == bos.BOS_FP32 else 'fp64'}" for n, p in CASES]

# Routes of the enum no plan can take on this hardware, with the reason; each entry is (factor route,
# predicate on the front's rows m) and the coverage test fails if a front matches one.
UNREACHED = {
    "pan64": ("pan64", lambda m: True,
              "the class-64 launch stays on the main stream only without the side stream, and mf_create "
              "fails when it cannot create it"),
    "blk": ("blk", lambda m: True,
            "mf_factor_blk stays on the main stream only without the second side stream (mf_create fails "
            "without it) or, with it, never: a level with blocked fronts forks whenever mf_factor_blk got its LDS"),
    "level_65_128": ("level", lambda m: m <= 128,
                     "mf_factor_level takes fronts of 65-128 rows (its LDS branch, m <= 90, among them) only "
                     "when mf_factor_blk cannot get its 129 KB of dynamic LDS (the !d->blk branch); a gfx950 CU "
                     "has 160 KB"),
}


def _handle(name, precision, graph=True):
    P, solver, leaf = solver_world(name)
    S = bos.Solver(P, precision=precision, solver=solver, schur_leaf=leaf, damping=SOLVER_DAMPING)
    if not graph:
        S.debug_set_step_graph(False)
    return P, S


@pytest.mark.parametrize("name,precision", CASES, ids=IDS)
def test_solve_matches_exact_answer(name, precision):
    P, S = _handle(name, precision)
    if precision == bos.BOS_FP32:
        info = S.system_info()
        assert info["pl_factored"] == 1 and info["fold_fp32"] == 1, info
    S.linearize()
    rows, cols, vals, b = S.export_system()
    st = S.step()
    assert st["solver_info"] == 0
    dx = S.last_dx()
    # the step built the very system exported before it
    rows2, cols2, vals2, b2 = S.export_system()
    S.close()
    assert np.array_equal(vals, vals2) and np.array_equal(b, b2)
    ref = solve_reference(rows, cols, vals, b, P.fixed)
    # the reference's sign (and the oracle's O.step): H dx = -b, the fixed pose's delta zero
    assert np.all(dx[3 * P.fixed:3 * P.fixed + 3] == 0.0)
    f, e, f_ref, e_ref, ok = ref.check(-dx[ref.idx], f"{name} {'fp32' if precision == bos.BOS_FP32 else 'fp64'} gpu")
    assert ok, (f, 4 * f_ref, e, 8 * e_ref)


@pytest.mark.parametrize("name,precision", CASES, ids=IDS)
def test_graph_replay_equals_individual_launches(name, precision):
    """Three steps as the captured graph's replay and as individual launches: the same bits."""
    out = []
    for graph in (True, False):
        P, S = _handle(name, precision, graph)
        dxs = []
        for _ in range(3):
            assert S.step()["solver_info"] == 0
            dxs.append(S.last_dx())
        out.append((dxs, S.get_state(), S.debug_solver_routes()))
        S.close()
    (dxa, (pa, la), ra), (dxb, (pb, lb), rb) = out
    for a, b in zip(dxa, dxb):
        assert np.array_equal(a, b)
    assert np.array_equal(pa, pb) and np.array_equal(la, lb)
    assert np.array_equal(ra, rb)


def test_every_route_is_covered():
    hit_f, hit_b = {}, {}
    fronts = []   # (case, factor route, backward route, k, m, folded children)
    for (name, precision), cid in zip(CASES, IDS):
        P, S = _handle(name, precision)
        with pytest.raises(bos.BosError, match=r"\(-1\)"):
            S.debug_solver_routes()   # nothing enqueued yet
        assert S.step()["solver_info"] == 0
        r = S.debug_solver_routes()
        stamps, meta = S.debug_solver_stamps(len(r))
        S.close()
        # every front is processed by one factor launch and one backward launch
        assert np.all((r[:, 0] >= 0) & (r[:, 0] < len(F))), (cid, r[(r[:, 0] < 0) | (r[:, 0] >= len(F))])
        assert np.all((r[:, 1] >= 0) & (r[:, 1] < len(B))), cid
        # the stamps hook agrees: sizes and the folded fronts; the dataflow launches stamped their fronts
        assert np.array_equal(meta[:, 1:3], r[:, 2:4])
        assert np.array_equal(meta[:, 0] == -1, r[:, 0] == F["folded"])
        assert np.array_equal(r[:, 0] == F["folded"], r[:, 1] == B["backward_fold"])
        assert np.all(stamps[0, r[:, 0] == F["flow"], 0] != 0) and np.all(stamps[1, r[:, 1] == B["backward_flow"], 0] != 0), cid
        for (rf, rb, k, rr), folds in zip(r.tolist(), meta[:, 3].tolist()):
            fronts.append((cid, rf, rb, k, k + rr, folds))
            hit_f.setdefault(rf, set()).add(cid)
            hit_b.setdefault(rb, set()).add(cid)
    for n, i in F.items():
        print(f"factor {n}: {sorted(hit_f.get(i, []))}")
    for n, i in B.items():
        print(f"backward {n}: {sorted(hit_b.get(i, []))}")
    whole = {n for n, (route, pred, _) in UNREACHED.items() if pred(1) and pred(10 ** 6)}
    for n, i in F.items():
        assert (i in hit_f) != (n in whole), f"factor route {n}: hit by {sorted(hit_f.get(i, []))}, UNREACHED {n in whole}"
    for n, i in B.items():
        assert i in hit_b, f"backward route {n} not hit"
    for n, (route, pred, why) in UNREACHED.items():
        assert why
        got = [f for f in fronts if f[1] == F[route] and pred(f[4])]
        assert not got, f"UNREACHED {n} is reached: {got[:3]}"
    # front sizes: wave kernels take m <= 64, the blocked ones 65-128, level the rest
    for cid, rf, rb, k, m, folds in fronts:
        name = bos.Solver.FACTOR_ROUTES[rf]
        if name in ("reg16", "reg16_side"):
            assert m <= 16, (cid, name, m)
        elif name == "pan48":
            assert 16 < m <= 48, (cid, m)
        elif name in ("pan64", "pan64_side"):
            assert 48 < m <= 64, (cid, m)
        elif name in ("blk", "blk_side2", "mixb_blk"):
            assert 64 < m <= 128, (cid, name, m)
        elif name == "mixb_wave":
            assert m <= 64, (cid, m)
        elif name == "level":
            assert m > 128, (cid, m)
        elif name == "flow":
            assert m <= 48, (cid, m)
        elif name == "folded":
            assert k == 2 and folds == 0, (cid, k)
    pan = [f for f in fronts if f[1] == F["pan48"]]
    assert any(f[3] <= 24 for f in pan) and any(f[3] > 24 for f in pan)      # the 24-column panel
    assert any(f[4] <= 32 for f in pan) and any(f[4] > 32 for f in pan)      # class-32 fronts ride along
    blk = [f for f in fronts if f[1] in (F["blk_side2"], F["mixb_blk"])]
    assert any(f[5] > 0 for f in blk) and any(f[5] == 0 for f in blk)        # with and without folded children
    for route in ("blk_side2", "mixb_blk", "mixb_wave", "pan48", "flow"):    # folds ride every kernel family
        print(f"{route}: fronts with folded children {sum(1 for f in fronts if f[1] == F[route] and f[5] > 0)}")
