"""Solver.jcbb() (bos_jcbb: J+H build, multifrontal factorization, the pair call's path solve and products, then
one wavefront per frame: S_all in LDS and the branch and bound in place) against the enumeration of
tests/jcbb_ref.py and bos.jcbb_search_host on the GPU's own innovation and innovation_cov, against
Solver.joint_compatibility() on the same handle, against the host twin, and for non-interference with the GN
steps around it. Frames, enumeration and checks: tests/jcbb_ref.py (the spurious frame's conditions: see
tests/test_jcbb_host.py)."""
import numpy as np
import pytest

import bos
import jcbb_ref as R
from conftest import C1, MINI
from helpers import gpu_lower
from joint_ref import JointReference
from marginals_ref import TOL_CAP, DenseInverses, sparse_tol
from test_edge_cov_host import edge_case_world
from test_jcbb_host import bad_calls

pytestmark = pytest.mark.gpu

SCHUR, SUPERNODAL = bos.BOS_SOLVER_SCHUR, bos.BOS_SOLVER_SUPERNODAL


@pytest.fixture(scope="module")
def c1():
    return bos.load_g2o(C1)


def _run(S, frames, batch=0, max_nodes=0, cov=True, detail=True):
    S.debug_set_jcbb_batch(batch)
    out = S.jcbb(frames, R.GATES, max_nodes=max_nodes, cov=cov, detail=detail)
    S.debug_set_jcbb_batch(0)
    assert out["solver_info"] == 0
    return out


def _frames(P, S):
    """The named frames at the handle's state, lists from the handle's own association"""
    def assoc(pose, z, om, k):
        o = S.associate_bearings(pose, z, om, gate=R.GATES[0], k=k)
        return o["cand_landmark"], o["cand_var"]

    def system(frame):
        o = _run(S, [frame])
        return o["innovation_cov"][0], o["innovation"]

    def systems(frames):
        o = _run(S, frames)
        return [(o["innovation_cov"][f], o["innovation"][R.frame_slices(o, f)[1]]) for f in range(len(frames))]

    return R.make_frames(P, S.get_state(), assoc, system, systems)


def _search_host(cands, S, e):
    return bos.jcbb_search_host(cands, S, e, R.GATES, max_nodes=1 << 26)


def _check_world(P, S, label, spurious_world=False, **plan):
    """The spurious frame's conditions first (asserted where the world has a pair with |rho| > SPURIOUS_RHO;
    spurious_world: it must be one); every frame against the enumeration or the host search on the GPU's own system;
    the joint call on the same handle; then the host twin on the GPU's exported values and state: the assignments
    agree on every frame that jcbb_ref.close_frames does not name, and it names at most one (twin, an exact tie)."""
    F = _frames(P, S)
    frames = R.frame_list(F)
    out = _run(S, frames)
    nodes = S.jcbb_timing()["nodes"]
    f = R.NAMES.index("spurious")
    holds = R.spurious_holds(F["spurious"][3], out["innovation_cov"][f], out["innovation"][R.frame_slices(out, f)[1]])
    print(f"  gpu {label} spurious: |rho| {F['spurious/rho']:.3f} (needed {R.SPURIOUS_RHO:.3f}); holds, paired, individually admissible, "
          f"gate cuts at depth >= 2: {holds}")
    assert F["spurious/rho"] > R.SPURIOUS_RHO or not spurious_world
    if F["spurious/rho"] > R.SPURIOUS_RHO:
        assert holds[0] and holds[1] < holds[2] and holds[3] >= 1
    for f, name in enumerate(R.NAMES):
        cands = F[name][3]
        big = R.leaves(cands) > R.BRUTE_LEAVES
        R.check_frame(out, f, cands, _search_host if big else None, f"{label} {name}")
        print(f"  gpu {label} {name}: m {len(cands)} P {sum(map(len, cands))} paired {out['n_paired'][f]} nis {out['joint_nis'][f]:.4g} nodes {nodes[f]}")
        assert big == (name in ("full", "deep")) or P.NL < 32
    R.check_against_joint(out, frames, lambda hyps: S.joint_compatibility(hyps, cov=True))
    # the host twin at the handle's state on the handle's exported values
    state = S.get_state()
    rows, cols, vals, _ = S.export_system()
    Q = bos.Problem(state[0], state[1], P.b_pose, P.b_lm, P.b_z, P.o_src, P.o_dst, P.o_z, P.o_omega, P.fixed, b_omega=P.b_omega,
                    pose_ids=P.pose_ids, lm_ids=P.lm_ids)
    host = bos.plan_mf_jcbb(Q, vals, frames, R.GATES, **plan)
    tol, _ = sparse_tol(P, gpu_lower(rows, cols, vals, P.N))
    close = R.close_frames(Q, vals, F, R.NAMES, out, min(tol, TOL_CAP), **plan)
    print(f"  gpu {label} vs host twin: closer than the bound (skipped): {close}")
    assert len(close) <= 1
    for f, name in enumerate(R.NAMES):
        if name not in close:
            b, _ = R.frame_slices(out, f)
            assert np.array_equal(out["assignment"][b], host["assignment"][b]) and out["n_paired"][f] == host["n_paired"][f], name
    return F, out


PLAN_KW = {"schur": dict(solver=SCHUR), "supernodal": dict(solver=SUPERNODAL), "schur_leaf40": dict(solver=SCHUR, schur_leaf=40)}


@pytest.mark.parametrize("plan", ["schur", "supernodal", "schur_leaf40"])
def test_c1(c1, plan):
    S = bos.Solver(c1, **PLAN_KW[plan])
    _check_world(c1, S, plan, spurious_world=True, **PLAN_KW[plan])
    S.close()


def test_mini_dataset():
    P = bos.load_g2o(MINI)
    S = bos.Solver(P)
    _check_world(P, S, "mini")
    S.close()


def test_register_class_alone():
    P = bos.synthetic(60, 120, 6)
    S = bos.Solver(P)
    _check_world(P, S, "synthetic 60/120/6")
    S.close()


def test_edge_case_world(c1):
    P = edge_case_world(c1)
    S = bos.Solver(P)
    _check_world(P, S, "edge cases")
    S.close()


def test_fp32(c1):
    S = bos.Solver(c1, precision=bos.BOS_FP32)
    _check_world(c1, S, "fp32")
    S.close()


def test_after_steps(c1):
    """At the estimate of 10 GN iterations."""
    S = bos.Solver(c1)
    S.step_n(10)
    _check_world(c1, S, "after 10 steps")
    S.close()


def test_all_pairings_accuracy(c1):
    """The all-pairings hypotheses of the frames against the dense inverse of the system the call linearised
    (JointReference.check): S_all and e_all are the joint call's, whose accuracy tests/test_gpu_joint.py pins."""
    S = bos.Solver(c1)
    F = _frames(c1, S)
    frames = [F[n] for n in ("clean", "two_poses", "fixed_pose")]
    out = _run(S, frames)
    state = S.get_state()
    rows, cols, vals, _ = S.export_system()
    Hl = gpu_lower(rows, cols, vals, c1.N)
    hyps = [R.all_pairings(fr) for fr in frames]
    res = S.joint_compatibility(hyps, cov=True)
    for f in range(len(frames)):
        assert np.array_equal(res["innovation_cov"][f], out["innovation_cov"][f])
    cat = lambda i: np.concatenate([h[i] for h in hyps])
    ref = JointReference(c1, Hl, res["hyp_start"], cat(0), cat(1), cat(2), cat(3), pose_xyt=state[0], lm_xy=state[1],
                         dense=DenseInverses(c1, Hl))
    ref.check(res, "gpu jcbb all-pairings")
    S.close()


@pytest.mark.parametrize("which", ["c1", "edge_cases"])
def test_exact_rules(c1, which):
    """Two calls, the repeated frame, order, company and one frame per batch: identical bits."""
    P = c1 if which == "c1" else edge_case_world(c1)
    S = bos.Solver(P)
    F = _frames(P, S)
    R.check_exact_rules(R.frame_list(F), lambda frames, batch=0: _run(S, frames, batch=batch))
    S.close()


def test_null_outputs_and_association_lists(c1):
    """A call with every detail output NULL returns the same assignment; without cov the rest is the same; lists
    fed straight from associate_bearings() with their -1 padding are the lists without it."""
    S = bos.Solver(c1)
    F = _frames(c1, S)
    frames = R.frame_list(F)
    full = _run(S, frames)
    lean = _run(S, frames, cov=False, detail=False)
    assert np.array_equal(lean["assignment"], full["assignment"])
    assert all(lean[k] is None for k in ("n_paired", "joint_nis", "prefix_nis", "complete", "innovation", "innovation_cov"))
    nocov = _run(S, frames, cov=False)
    for k in ("assignment", "n_paired", "joint_nis", "prefix_nis", "complete", "innovation"):
        assert np.array_equal(nocov[k], full[k]), k
    pose, z, om, cands = F["clean"]
    a = S.associate_bearings(pose, z, om, gate=0.01, k=4)          # a gate of 0.1 standard deviations: short lists
    assert (a["cand_landmark"] == -1).any() and (a["cand_landmark"][:, 0] >= 0).all()
    padded = _run(S, [(pose, z, om, a["cand_landmark"])])
    listed = _run(S, [(pose, z, om, [[int(l) for l in row if l >= 0] for row in a["cand_landmark"]])])
    R.same_frame(padded, 0, listed, 0)
    assert padded["n_paired"][0] >= 1 and padded["complete"][0] == 1
    t = S.jcbb_timing()
    assert t["jcbb_bytes"] > 0 and t["factor_ms"] > 0 and t["path_ms"] > 0 and t["search_ms"] > 0 and len(t["nodes"]) == 1 and t["nodes"][0] > 0
    S.close()


@pytest.mark.parametrize("budget", [1, 50])
def test_budget(c1, budget):
    """An exhausted budget gives complete == 0 and an admissible hypothesis (re-checked through ldl_prefix on the
    frame's own system); frames that finish inside it are the full search's."""
    from test_jcbb_host import _admissible
    S = bos.Solver(c1)
    F = _frames(c1, S)
    names = R.NAMES + ("moved",)                                 # moved: the long search (180 nodes)
    frames = [F[n] for n in names]
    full = _run(S, frames)
    need = S.jcbb_timing()["nodes"].copy()
    out = _run(S, frames, max_nodes=budget)
    nodes = S.jcbb_timing()["nodes"]
    assert np.all(nodes <= budget) and need[-1] > 50
    for f, name in enumerate(names):
        _admissible(frames[f], out, f)
        if need[f] > budget:
            assert out["complete"][f] == 0, name
        else:
            R.same_frame(full, f, out, f)
    S.close()


@pytest.mark.parametrize("precision", [bos.BOS_FP64, bos.BOS_FP32])
def test_steps_do_not_see_the_call(c1, precision):
    """The state is bit-identical across jcbb(); step, call, step ends where step, step does."""
    A = bos.Solver(c1, precision=precision)
    B = bos.Solver(c1, precision=precision)
    A.step()
    B.step()
    before = A.get_state()
    F = _frames(c1, A)
    _run(A, R.frame_list(F))
    after = A.get_state()
    assert np.array_equal(before[0], after[0]) and np.array_equal(before[1], after[1])
    with pytest.raises(bos.BosError, match=r"\(-1\)"):
        A.last_dx()                                              # as after bos_marginals
    sa = A.step()
    sb = B.step()
    pa, la = A.get_state()
    pb, lb = B.get_state()
    A.close()
    B.close()
    assert np.array_equal(pa, pb) and np.array_equal(la, lb)
    assert sa["chi2"] == sb["chi2"] and sa["solver_info"] == sb["solver_info"] == 0


def test_empty_call_and_bad_arguments(c1):
    S = bos.Solver(c1)
    S.step()
    dx = S.last_dx()
    out = S.jcbb([], R.GATES)
    assert len(out["n_paired"]) == 0 and out["solver_info"] == 0
    assert np.array_equal(S.last_dx(), dx)                       # n_frames = 0 touched nothing
    for name, (raw, gate, max_nodes) in bad_calls(c1.NP, c1.NL).items():
        with pytest.raises(bos.BosError, match=r"\(-1\).*bos_jcbb"):
            S.jcbb(raw, gate, max_nodes=max_nodes)
    assert np.array_equal(S.last_dx(), dx)
    with pytest.raises(bos.BosError, match=r"\(-1\)"):
        S.debug_set_jcbb_batch(-1)
    S.close()


@pytest.mark.parametrize("kind", ["dense", "rf", "communicator"])
def test_unsupported_handles(c1, kind):
    kw = {"dense": dict(solver=bos.BOS_SOLVER_DENSE_CHOL), "rf": dict(solver=bos.BOS_SOLVER_ROCSOLVER_RF),
          "communicator": dict(solver=SCHUR, rank=0, world_size=1, nccl_id=bos.nccl_unique_id())}[kind]
    S = bos.Solver(c1, **kw)
    with pytest.raises(bos.BosError, match=r"\(-5\).*bos_jcbb"):
        S.jcbb([([1], [0.1], None, [[0]])], R.GATES)
    S.close()
