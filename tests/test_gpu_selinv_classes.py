"""The selected inverse (hip/selinv.hip selinv_front<T, X>) against a refined dense inverse, front class
by front class.

Every front takes one of three code paths, chosen by selinv_build: one wavefront with the working set in
LDS, 256 threads with the working set in LDS and G Z on f64 MFMA tiles, or 256 threads with Li / Z / S_RJ
in the global workspace; each with and without the cross blocks' emission (X). Each case here is one
world of test_selinv_criterion_host.SELINV_CASES (the solver route tests' worlds, one world with a
128-row front, and the reference dataset's three plans); the class of every front is read from
selinv_build's own report (Solver.debug_selinv_fronts), and test_every_class_and_shape_is_covered
fails when a class, shape or record kind of COVERAGE_ITEMS is not taken by a front whose outputs were
compared, or when an UNREACHED one is.

Criterion (marginals_ref.py, edge_cov_ref.py): one edge_covariances(), export_system() and get_state()
at the same state. Sigma* is the dense inverse of the exported system refined in np.longdouble; the
device's blocks, cross blocks and projected covariances pass when their scaled error is within 8 x the
larger error of two plain fp64 inverses (LU, Cholesky) of that very system, over the same entries. The
errors are attributed to the front that wrote them and the worst ratio is printed per class. An fp32
handle exports exactly the values its factorization reads (tests/test_gpu_solver_routes.py), so the
criterion applies to its own export. marginals() on the same handle must return the diagonal blocks'
bits: the X = false instance against the X = true one in every class."""
import hashlib

import numpy as np
import pytest

import bos
from edge_cov_ref import RefinedEdgeReference, check_reference, check_refined, check_structure
from helpers import SOLVER_DAMPING, gpu_lower
from marginals_ref import MARGIN, TOL_CAP, check_blocks, ratio
from test_selinv_criterion_host import (FP32_SCHUR_WORLD, SELINV_CASES, check_coverage, front_records,
                                        predicted_class, selinv_case)

pytestmark = pytest.mark.gpu

CLASSES = bos.Solver.SELINV_CLASSES
CASES = [(n, bos.BOS_FP64) for n in sorted(SELINV_CASES)] + [(FP32_SCHUR_WORLD, bos.BOS_FP32), ("150_sn", bos.BOS_FP32)]
IDS = [f"{n}-{'fp32' if p == bos.BOS_FP32 else 'fp64'}" for n, p in CASES]
COL = {n: i for i, n in enumerate(bos.Solver.SELINV_COLS)}
_refs, _runs = {}, {}


def _reference(P, rows, cols, vals, pose, lm):
    """The refined reference of an exported system and state, computed once per distinct system (the
    reference dataset's three plans export the same H)."""
    Hl = gpu_lower(rows, cols, vals, P.N)
    Hl.sum_duplicates()
    Hl.sort_indices()
    key = hashlib.sha1(b"".join(np.ascontiguousarray(a).tobytes() for a in (Hl.indptr, Hl.indices, Hl.data, pose, lm))).hexdigest()
    if key not in _refs:
        _refs[key] = RefinedEdgeReference(P, Hl, pose, lm)
    return _refs[key]


def _run(name, precision):
    """One case, run once: the handle's results, its report, the reference and the attributed errors."""
    if (name, precision) in _runs:
        return _runs[(name, precision)]
    _, P, solver, leaf = selinv_case(name)
    S = bos.Solver(P, precision=precision, solver=solver, schur_leaf=leaf, damping=SOLVER_DAMPING)
    if precision == bos.BOS_FP32 and solver == bos.BOS_SOLVER_SCHUR:
        info = S.system_info()
        assert info["pl_factored"] == 1 and info["fold_fp32"] == 1, info
    with pytest.raises(bos.BosError, match=r"\(-1\)"):
        S.debug_selinv_fronts()   # no plan built yet
    out = S.edge_covariances()
    rows, cols, vals, _ = S.export_system()
    pose, lm = S.get_state()
    report = S.debug_selinv_fronts()
    mpose, mlm, minfo = S.marginals()
    report2 = S.debug_selinv_fronts()
    S.close()
    assert out["solver_info"] == 0 and minfo == 0
    ref = _reference(P, rows, cols, vals, pose, lm)
    run = dict(P=P, solver=solver, leaf=leaf, out=out, report=report, report2=report2, marginals=(mpose, mlm), ref=ref)
    _runs[(name, precision)] = run
    return run


def _by_class(run, errs):
    """{group: {class: worst error}}: block errors by the front that wrote the node's block, cross and
    projected errors by the front that emitted the edge's cross block (an edge from the fixed pose has
    no cross block: its projected entry comes from the other node's block, and goes to that front)."""
    P, rep = run["P"], run["report"]
    cls = rep["fronts"][:, COL["class"]]
    node, edge = rep["node_front"], rep["edge_front"]
    a = np.concatenate([P.b_pose, P.o_src])
    b = np.concatenate([P.NP + P.b_lm, P.o_dst])
    proj = np.where(edge >= 0, edge, np.where(a == P.fixed, node[b], node[a]))
    out = {}
    for group, front in (("blocks", node), ("cross", edge), ("projected", proj)):
        e, worst = errs[group], {}
        assert len(e) == len(front)
        for c, cname in enumerate(CLASSES):
            sel = (front >= 0) & (cls[np.maximum(front, 0)] == c)
            if sel.any():
                worst[cname] = float(e[sel].max())
        assert np.all(e[front < 0] == 0.0)       # the fixed pose's block and edges: exactly zero, nothing to attribute
        out[group] = worst
    return out


@pytest.mark.parametrize("name,precision", CASES, ids=IDS)
def test_every_class_matches_the_refined_inverse(name, precision):
    run = _run(name, precision)
    P, out, ref = run["P"], run["out"], run["ref"]
    print(f"selinv classes gpu {name} {'fp32' if precision == bos.BOS_FP32 else 'fp64'}: n {ref.n} residual {ref.residual:.3g}")
    assert ref.residual <= 1e-9
    # per class first, so that a failing case says which class produced its error
    errs = {"blocks": ref.refined.errors(out["pose_cov"], out["landmark_cov"]),
            "cross": ref.edge_errors("cross", out), "projected": ref.edge_errors("projected", out)}
    for group, worst in _by_class(run, errs).items():
        for cname, e in worst.items():
            print(f"  class {cname} {group}: e {e:.3g} ratio {ratio(e, ref.e_ref[group]):.3g}")
    check_refined(ref, out, f"gpu {name}")
    check_reference(ref, out, TOL_CAP)
    check_blocks(P, out["pose_cov"], out["landmark_cov"])
    check_structure(P, out)
    # X = false against X = true, every class: the marginals' launches give the same bits
    assert np.array_equal(run["marginals"][0], out["pose_cov"]) and np.array_equal(run["marginals"][1], out["landmark_cov"])


@pytest.mark.parametrize("name,precision", CASES, ids=IDS)
def test_report_agrees_with_the_plan(name, precision):
    """The device's report against the plan's own listing (bos.plan_mf_fronts): shapes, folds, Sigma
    fronts and record counts; classes as the front size predicts on a device that grants the large LDS;
    every node and every edge off the fixed pose attributed to a front that holds its record."""
    run = _run(name, precision)
    P, rep = run["P"], run["report"]
    f, plan = rep["fronts"], bos.plan_mf_fronts(P, solver=run["solver"], schur_leaf=run["leaf"])
    PC = {n: i for i, n in enumerate(bos.PLAN_FRONT_COLS)}
    assert all(np.array_equal(run["report2"][k], rep[k]) for k in rep)      # marginals() changes nothing
    assert len(f) == len(plan)
    for a, b in (("k", "k"), ("r", "r"), ("folded", "folded"), ("diag_records", "diag_records"), ("cross_rj", "cross_rj"),
                 ("cross_jj", "cross_jj"), ("cross_transposed", "cross_transposed")):
        assert np.array_equal(f[:, COL[a]], plan[:, PC[b]]), a
    assert np.array_equal(f[:, COL["sigma_front"]], (plan[:, PC["children"]] > 0).astype(np.int32))
    assert [CLASSES[c] for c in f[:, COL["class"]]] == [predicted_class(int(m)) for m in f[:, COL["k"]] + f[:, COL["r"]]]
    # launches: top-down by level, the folded landmarks last; a front's launch follows its parent's
    launch, parent = f[:, COL["launch"]], plan[:, PC["parent"]]
    assert np.all(launch >= 0)
    has = parent >= 0
    assert np.all(launch[has] > launch[parent[has]])
    for ln in np.unique(launch):
        assert len(set(f[launch == ln, COL["class"]] == 0)) == 1            # one thread count per launch
    node, edge = rep["node_front"], rep["edge_front"]
    free = np.arange(P.NP + P.NL) != P.fixed
    assert node[P.fixed] == -1 and np.all(node[free] >= 0)
    assert np.array_equal(np.bincount(node[free], minlength=len(f)), f[:, COL["diag_records"]])
    fixed_edge = np.concatenate([P.b_pose == P.fixed, (P.o_src == P.fixed) | (P.o_dst == P.fixed)])
    assert np.all(edge[fixed_edge] == -1) and np.all(edge[~fixed_edge] >= 0)
    # an edge's cross block comes from the front of the node eliminated first: one of its two nodes' fronts
    a = np.concatenate([P.b_pose, P.o_src])
    b = np.concatenate([P.NP + P.b_lm, P.o_dst])
    ok = (edge == node[a]) | (edge == node[b])
    assert np.all(ok[~fixed_edge])


def test_every_class_and_shape_is_covered():
    recs = []
    worst = {c: {} for c in CLASSES}
    for (name, precision), cid in zip(CASES, IDS):
        run = _run(name, precision)
        P, rep, ref, out = run["P"], run["report"], run["ref"], run["out"]
        f = rep["fronts"]
        errs = {"blocks": ref.refined.errors(out["pose_cov"], out["landmark_cov"]),
                "cross": ref.edge_errors("cross", out), "projected": ref.edge_errors("projected", out)}
        for group, w in _by_class(run, errs).items():
            for cname, e in w.items():
                r = ratio(e, ref.e_ref[group])
                if r > worst[cname].get(group, (-1.0,))[0]:
                    worst[cname][group] = (r, cid)
        # a front's outputs were compared when a node's block or an edge's cross block is attributed to it
        compared = np.zeros(len(f), dtype=bool)
        compared[rep["node_front"][rep["node_front"] >= 0]] = True
        compared[rep["edge_front"][rep["edge_front"] >= 0]] = True
        plan = bos.plan_mf_fronts(P, solver=run["solver"], schur_leaf=run["leaf"])
        recs += front_records(cid, plan, classes=[CLASSES[c] for c in f[:, COL["class"]]], compared=compared)
    for cname in CLASSES:
        cases = sorted({f.case for f in recs if f.cls == cname})
        print(f"class {cname}: cases {cases}")
        for group in ("blocks", "cross", "projected"):
            r, cid = worst[cname][group]
            print(f"  worst {group} ratio {r:.3g} ({cid})")
            assert r <= MARGIN
    check_coverage(recs)
