"""The refined selected-inverse criterion (marginals_ref.RefinedReference, edge_cov_ref.RefinedEdgeReference:
Sigma* refined in np.longdouble, the bound 8 e_ref measured from two plain fp64 inverses of the same H)
on the host twin, the front shapes the GPU class tests rely on, and the gap the criterion closes.

The cases (SELINV_CASES) are shared with tests/test_gpu_selinv_classes.py: the nine worlds of
helpers.SOLVER_WORLDS, one world local to these two files whose nested-dissection plan has a front of
exactly 128 rows (found by a seed search over bos.synthetic with bos.plan_mf_fronts), and the reference
dataset's three plans. H is the oracle's at SOLVER_DAMPING."""
import types

import numpy as np
import pytest

import bos
import oracle as O
from conftest import C1
from edge_cov_ref import RefinedEdgeReference, check_reference, check_refined, check_structure
from helpers import SOLVER_DAMPING, SOLVER_WORLDS, oracle_lower_nf, solver_world, to_oracle
from marginals_ref import MARGIN, TOL_CAP, check_blocks

SCHUR, SUPERNODAL = bos.BOS_SOLVER_SCHUR, bos.BOS_SOLVER_SUPERNODAL
CLASSES = bos.Solver.SELINV_CLASSES

# name -> (dataset key, solver, schur_leaf); the dataset is built once (selinv_case)
SELINV_CASES = {n: (n, s, leaf) for n, (_, s, leaf) in SOLVER_WORLDS.items()}
SELINV_CASES["62_sn_m128"] = ("62_9_3_seed2", SUPERNODAL, 0)      # a (72, 56) front: m = 128
SELINV_CASES["c1_schur"] = ("c1", SCHUR, 0)
SELINV_CASES["c1_sn"] = ("c1", SUPERNODAL, 0)
SELINV_CASES["c1_schur_leaf40"] = ("c1", SCHUR, 40)
_data, _refs = {}, {}


def selinv_case(name):
    """(dataset key, problem, solver, schur_leaf) of a SELINV_CASES entry."""
    key, solver, leaf = SELINV_CASES[name]
    if key not in _data:
        _data[key] = (solver_world(key)[0] if key in SOLVER_WORLDS else
                      bos.load_g2o(C1) if key == "c1" else bos.synthetic(62, 9, 3, seed=2))
    return key, _data[key], solver, leaf


def _oracle_reference(key, P):
    """The oracle's lower H_nf of a dataset and its refined reference (J at P's state), computed once."""
    if key not in _refs:
        Q = to_oracle(P)
        Hl = oracle_lower_nf(Q, O.linearize(Q, damping=SOLVER_DAMPING)).tocsr()
        _refs[key] = (Hl, RefinedEdgeReference(P, Hl))
    return _refs[key]


def _host_twin(name):
    key, P, solver, leaf = selinv_case(name)
    Hl, ref = _oracle_reference(key, P)
    info = bos.plan_inspect(P, 0, 1, entries=True, solver=solver, schur_leaf=leaf)
    vals = np.asarray(Hl[info["rows"], info["cols"]]).ravel()
    return P, ref, bos.plan_mf_edge_covariances(P, vals, solver=solver, schur_leaf=leaf)


@pytest.mark.parametrize("name", sorted(SELINV_CASES))
def test_host_twin_passes_the_refined_criterion(name):
    """Blocks, cross blocks and projected entries of the host twin within 8 e_ref of Sigma*, beside the
    old bounds and the exact-structure checks. The Newton step's residual max |I - H X0| stays below
    1e-9: its square, the step's own truncation, is then far below the fp64 references' error."""
    P, ref, out = _host_twin(name)
    print(f"selinv criterion host {name}: n {ref.n} residual {ref.residual:.3g}")
    assert ref.residual <= 1e-9
    check_reference(ref, out, TOL_CAP)
    check_refined(ref, out, f"host {name}")
    check_blocks(P, out["pose_cov"], out["landmark_cov"])
    check_structure(P, out)


WAVE_MAX_M, BLK_MAX_M = 64, 128   # csrc/host/plan.hpp kMfWaveMaxM, kMfBlkMaxM


def predicted_class(m):
    """The class selinv_build gives a front of m rows on a device that grants the 128 KiB of LDS."""
    return CLASSES[0 if m <= WAVE_MAX_M else 1 if m <= BLK_MAX_M else 2]


def front_records(case, plan_fronts, classes=None, compared=None):
    """One record per front of a case for the coverage items below. plan_fronts: bos.plan_mf_fronts;
    classes: the class name of every front (the device's report; predicted from m when None); compared:
    per front, whether one of its outputs was compared with a reference (all when None)."""
    C = {n: i for i, n in enumerate(bos.PLAN_FRONT_COLS)}
    f = np.asarray(plan_fronts)
    cls = [predicted_class(int(k + r)) for k, r in f[:, :2]] if classes is None else list(classes)
    recs = []
    for s, row in enumerate(f.tolist()):
        if compared is not None and not compared[s]:
            continue
        k, r, parent = row[C["k"]], row[C["r"]], row[C["parent"]]
        kids = np.nonzero(f[:, C["parent"]] == s)[0]
        recs.append(types.SimpleNamespace(
            case=case, s=s, cls=cls[s], k=k, r=r, m=k + r, folded=bool(row[C["folded"]]), children=row[C["children"]],
            folded_children=row[C["folded_children"]], parent_cls=cls[parent] if parent >= 0 else None,
            child_cls={cls[c] for c in kids}, tiles=-(-r // 16) * -(-k // 16), rj=row[C["cross_rj"]],
            jj=row[C["cross_jj"]], tr=row[C["cross_transposed"]], diag=row[C["diag_records"]]))
    return recs


def _items():
    W, B, G = CLASSES
    it = {
        "wave: a root": lambda f: f.cls == W and f.r == 0,
        "wave: a folded front": lambda f: f.cls == W and f.folded,
        "wave: not folded, k > 16": lambda f: f.cls == W and not f.folded and f.k > 16,
        "wave: m = 64": lambda f: f.cls == W and f.m == 64,
        "blocked: a root": lambda f: f.cls == B and f.r == 0,
        "blocked: r % 4 != 0": lambda f: f.cls == B and f.r % 4 != 0,
        "blocked: r % 16 == 0": lambda f: f.cls == B and f.r > 0 and f.r % 16 == 0,
        "blocked: k <= 16": lambda f: f.cls == B and f.k <= 16,
        "blocked: 16 < k <= 32": lambda f: f.cls == B and 16 < f.k <= 32,
        "blocked: k > 32": lambda f: f.cls == B and f.k > 32,
        "blocked: more than 4 tiles": lambda f: f.cls == B and f.tiles > 4,
        "blocked: 1 to 4 tiles": lambda f: f.cls == B and 1 <= f.tiles <= 4,
        "blocked: m = 65": lambda f: f.cls == B and f.m == 65,
        "blocked: m = 128": lambda f: f.cls == B and f.m == 128,
        "blocked: folded children": lambda f: f.cls == B and f.folded_children > 0,
        "blocked: the parent is blocked too": lambda f: f.cls == B and f.parent_cls == B,
        "workspace: a root": lambda f: f.cls == G and f.r == 0,
        "workspace: a k = 2 landmark leaf": lambda f: f.cls == G and f.k == 2 and f.children == 0,
        "workspace: r > k": lambda f: f.cls == G and f.r > f.k,
        "workspace: k > r": lambda f: f.cls == G and f.k > f.r,
        "workspace: m = 129": lambda f: f.cls == G and f.m == 129,
        "workspace: wave children read its Sigma front": lambda f: f.cls == G and W in f.child_cls,
    }
    for c in CLASSES:
        it[f"{c}: a Sigma_RJ cross record"] = lambda f, c=c: f.cls == c and f.rj > 0
        it[f"{c}: a Sigma_JJ cross record"] = lambda f, c=c: f.cls == c and f.jj > 0
        it[f"{c}: a transposed cross record"] = lambda f, c=c: f.cls == c and f.tr > 0
    return it


# what test_every_class_and_shape_is_covered (GPU) asserts of the fronts whose outputs it compared, and
# the test below of the plans alone
COVERAGE_ITEMS = _items()
# cases no plan can reach on this hardware: name -> (predicate, reason); reaching one fails the test
UNREACHED = {
    "blocked front without the large LDS": (
        lambda f: f.cls == CLASSES[2] and f.m <= BLK_MAX_M,
        "a front of 65-128 rows goes to the workspace class only when hipFuncSetAttribute refuses selinv_front's "
        "128 KiB of dynamic LDS; a gfx950 CU has 160 KiB"),
}


def check_coverage(recs):
    """Every COVERAGE_ITEMS entry is hit by a record, no UNREACHED entry is; prints who hits what."""
    for name, pred in COVERAGE_ITEMS.items():
        hit = sorted({f.case for f in recs if pred(f)})
        print(f"{name}: {hit}")
        assert hit, f"no compared front is: {name}"
    for name, (pred, why) in UNREACHED.items():
        assert why
        got = [(f.case, f.s, f.k, f.r) for f in recs if pred(f)]
        assert not got, f"UNREACHED {name} is reached: {got[:3]}"


def test_plans_have_the_shapes_the_gpu_coverage_relies_on():
    """From the plans alone (bos.plan_mf_fronts, the class predicted from m): the cases reach every
    class, shape and record kind of COVERAGE_ITEMS, and the fp32 cases' Schur world folds from fp32."""
    recs = []
    for name in sorted(SELINV_CASES):
        _, P, solver, leaf = selinv_case(name)
        f = bos.plan_mf_fronts(P, solver=solver, schur_leaf=leaf)
        info = bos.plan_inspect(P, solver=solver, schur_leaf=leaf)
        assert len(f) == info["mf_supernodes"] and int((f[:, 0] + f[:, 1]).max()) == info["mf_max_front"]
        assert int(f[:, 0].sum()) == info["n"] and np.all(f[f[:, 6] == 1, 0] == 2)
        assert int(f[:, 7].sum()) == P.NP + P.NL - 1          # every node but the fixed pose in one record
        recs += front_records(name, f)
    check_coverage(recs)
    _, P, solver, leaf = selinv_case(FP32_SCHUR_WORLD)
    assert solver == SCHUR and bos.plan_inspect(P, solver=solver, schur_leaf=leaf)["mf_fold_fp32"]


FP32_SCHUR_WORLD = "100_schur_leaf30"   # blocked fronts with folded children: the folds read fp32 blocks
MUTATED_WORLD = "150_sn"


@pytest.mark.parametrize("what", ["block", "cross", "projected"])
def test_criterion_rejects_one_entry_off_by_1e_9(what):
    """The gap this criterion closes, kept as a test: one entry of the host twin's result moved by 1e-9
    of its scale passes the old bound (tol >= 1e-8 on this world) and fails the refined one."""
    P, ref, out = _host_twin(MUTATED_WORLD)
    assert 1e-8 <= ref.tol <= TOL_CAP and 1e-9 > 2 * MARGIN * max(ref.e_ref.values())
    bad = {k: v.copy() for k, v in out.items()}
    if what == "block":
        u = next(u for u in range(P.NP) if u != P.fixed)
        bad["pose_cov"][u, 1, 1] += 1e-9 * float(ref.refined.sd[3 * u + 1]) ** 2
    elif what == "cross":
        e = next(e for e in range(len(P.o_z)) if P.fixed not in (P.o_src[e], P.o_dst[e]) and P.o_src[e] != P.o_dst[e])
        bad["odom_cross"][e, 2, 0] += 1e-9 * float(ref.star_scale["odom_cross"][e, 2, 0])
    else:
        e = next(e for e in range(len(P.b_z)) if P.b_pose[e] != P.fixed)
        bad["bearing_var"][e] += 1e-9 * float(ref.star_scale["bearing_var"][e])
    check_reference(ref, bad, TOL_CAP)          # the old bound accepts it
    check_refined(ref, out, "unmutated")
    with pytest.raises(AssertionError):
        check_refined(ref, bad, f"mutated {what}")
