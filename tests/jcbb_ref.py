"""Reference, frames and checks shared by the JCBB tests (host and GPU).

brute_force enumerates every assignment of a frame (itertools.product over each bearing's list plus "nothing"),
drops those that use a landmark twice, evaluates joint_ref.ldl_prefix on the principal submatrix of S_all and
the subvector of e_all, tests admissibility (every prefix finite and <= gate[j - 1]) and applies the total order
of bos.h bos_jcbb: most pairings, then smallest joint NIS, then the lexicographically smallest choice vector
(list positions, nothing after every position). It prunes nothing.

Frames (make_frames) are built at a state for a free pose a with as many observed landmarks as the world has
(six and more on C1), omega = OMEGA for every bearing, candidate lists from a k = 3 association at the gate of
one degree of freedom unless said otherwise:
  clean          z = the predicted bearing of the true landmarks + 0.002 (-1)^b: all m paired
  spurious       two bearings with one candidate each, from the pose and the pair of its observed landmarks whose
                 innovations are most correlated (largest |rho| over every free pose, found by one call: systems(frames)), the second z moved by the first offset of SPURIOUS_OFFSETS (in sqrt(S_ii)) for which
                 the enumeration on the frame's own system says: inside its own gate, rejected by the joint test
                 (spurious_holds). Two pairings with single NIS t and ~0 have the joint NIS t / (1 - rho^2), so with
                 t = 1.9^2 <= gate[0] the second gate rejects iff |rho| > SPURIOUS_RHO = sqrt(1 - 1.9^2 / gate[1]) =
                 0.630: C1 has such a pair (0.68), mini and synthetic(60, 120, 6) have none (|rho| < 0.003), and
                 there the last offset tried is kept. F["spurious/rho"] is the pair's |rho|
  conflict       two bearings, 0.004 apart, whose first candidate is the same landmark (the second one's list
                 is reordered to begin with the first one's first candidate)
  twin           two bit-identical bearings, each with the single candidate X: (X, nothing) by the
                 lexicographic rule, an exact NIS tie
  no_candidates  clean with two lists emptied
  empty          m = 0
  fixed_pose     bearings from the fixed pose
  two_poses      bearings from two poses in one frame
  full           P = 32 as 8 x 4 (fewer where the world has fewer landmarks): the true landmark first, then the
                 next three of the pose's list
  deep           20 bearings x 1 candidate + 6 x 2: depth 26, P = 32 (scaled down where the world is smaller)
"""
import itertools

import numpy as np
from scipy.stats import chi2

import bos
from associate_ref import predicted_bearings
from joint_ref import ldl_prefix

GATES = chi2.ppf(0.95, np.arange(1, bos.JOINT_MAX_M + 1))
OMEGA = 1e4
BRUTE_LEAVES = 4096
NOTHING = np.iinfo(np.int32).max


def leaves(cands):
    n = 1
    for c in cands:
        n *= len(c) + 1
    return n


def brute_force(cands, S, e, gate=GATES):
    """The result of one frame by enumeration: dict with assignment [m], choice (tuple), n_paired, joint_nis,
    prefix_nis [m], pairings (the winner's, as indices into the frame's pairings), runner_up (the second hypothesis by
    the order: (n_paired, joint_nis) or None) and runner_up_pairings, gate_cuts_deep
    (hypotheses whose first failing prefix is the j-th, j >= 2) and admissible (their number)."""
    m = len(cands)
    start = np.concatenate([[0], np.cumsum([len(c) for c in cands])]).astype(int)
    S, e = np.asarray(S, dtype=np.float64), np.asarray(e, dtype=np.float64)
    ranked, deep = [], 0
    for choice in itertools.product(*[range(len(c) + 1) for c in cands]):
        lms = [cands[b][c] for b, c in enumerate(choice) if c < len(cands[b])]
        if len(set(lms)) != len(lms):
            continue
        q = [start[b] + c for b, c in enumerate(choice) if c < len(cands[b])]
        pre = ldl_prefix(S[np.ix_(q, q)], e[q]) if q else np.zeros(0)
        ok = [bool(np.isfinite(p) and p <= gate[j]) for j, p in enumerate(pre)]
        if not all(ok):
            if ok.index(False) >= 1:
                deep += 1
            continue
        key = tuple(c if c < len(cands[b]) else NOTHING for b, c in enumerate(choice))
        ranked.append((-len(q), float(pre[-1]) if q else 0.0, key, pre, q))
    ranked.sort(key=lambda r: r[:3])
    n, nis, key, pre, q = ranked[0]
    prefix, j = np.zeros(m), 0
    for b in range(m):
        if key[b] != NOTHING:
            j += 1
        prefix[b] = pre[j - 1] if j else 0.0
    return {"assignment": np.array([cands[b][c] if c != NOTHING else -1 for b, c in enumerate(key)], dtype=np.int32),
            "choice": key, "n_paired": -n, "joint_nis": nis, "prefix_nis": prefix,
            "pairings": q, "runner_up": (-ranked[1][0], ranked[1][1]) if len(ranked) > 1 else None,
            "runner_up_pairings": ranked[1][4] if len(ranked) > 1 else None, "gate_cuts_deep": deep,
            "admissible": len(ranked)}


def observed(P, a):
    return [int(l) for l in np.unique(P.b_lm[P.b_pose == a])]


SPURIOUS_OFFSETS = (1.9, -1.9, 1.8, -1.8)
SPURIOUS_RHO = float(np.sqrt(1.0 - 1.9 ** 2 / GATES[1]))


def spurious_holds(cands, S, e, gate=GATES):
    """(holds, winner's pairings, bearings with an individually admissible candidate, gate cuts at depth >= 2):
    what the spurious frame is for, from the enumeration."""
    start = np.concatenate([[0], np.cumsum([len(c) for c in cands])]).astype(int)
    alone = sum(any(S[q, q] > 0 and e[q] * e[q] / S[q, q] <= gate[0] for q in range(start[b], start[b + 1])) for b in range(len(cands)))
    ref = brute_force(cands, S, e, gate)
    return ref["n_paired"] < alone and ref["gate_cuts_deep"] >= 1, ref["n_paired"], alone, ref["gate_cuts_deep"]


def make_frames(P, state, assoc, system, systems=None):
    """name -> (pose [m], z [m], omega [m], candidates: list of lists). assoc(pose, z, omega, k) -> (cand_landmark
    [n, k] with -1 padding, cand_var [n, k]) at the gate of one degree of freedom; system(frame) -> (S_all, e_all)
    of one frame; systems(frames) -> the list of them for several frames in one call."""
    pose_xyt, lm_xy = state
    systems = systems or (lambda frames: [system(fr) for fr in frames])
    free = [p for p in range(P.NP) if p != P.fixed]
    a = max(free, key=lambda p: (len(observed(P, p)), -p))
    obs = observed(P, a)
    others = [l for l in range(P.NL) if l not in obs]
    pred = lambda p, l: float(predicted_bearings(pose_xyt, lm_xy, int(p))[int(l)])
    lists = lambda cl: [[int(l) for l in row if l >= 0] for row in cl]
    F = {}

    def frame(name, poses, lms, offsets, cands=None, k=3):
        poses = np.asarray(poses, dtype=np.int32)
        z = np.array([pred(p, l) + d for p, l, d in zip(poses, lms, offsets)])
        om = np.full(len(z), OMEGA)
        if cands is None:
            cl, var = assoc(poses, z, om, k) if len(z) else (np.zeros((0, k), dtype=np.int32), np.zeros((0, k)))
            cands, F[name + "/var"] = lists(cl), var
        F[name] = (poses, z, om, cands)

    m = min(5, len(obs))
    alt = lambda n: [0.002 * (-1) ** b for b in range(n)]
    frame("clean", [a] * m, obs[:m], alt(m))
    # spurious: the most correlated pair of one pose's observed landmarks, the second bearing moved
    best = (-1.0, a, obs[0], obs[min(1, len(obs) - 1)], 1.0)
    scan = [p for p in free if len(observed(P, p)) >= 2]
    for p in scan:
        seen = observed(P, p)[:bos.JOINT_MAX_M]
        frame(f"scan/{p}", [p] * len(seen), seen, [0.0] * len(seen), cands=[[l] for l in seen])
    for p, (S, _) in zip(scan, systems([F[f"scan/{p}"] for p in scan])):
        seen = observed(P, p)[:bos.JOINT_MAX_M]
        d = np.sqrt(np.diag(S))
        rho = np.abs(np.tril(S / np.outer(d, d), -1))
        i, j = np.unravel_index(np.argmax(rho), rho.shape)
        if rho[i, j] > best[0]:
            best = (float(rho[i, j]), p, seen[j], seen[i], float(d[i]))
    F["spurious/rho"], p, la, lb, sd = best
    for mult in SPURIOUS_OFFSETS:
        frame("spurious", [p, p], [la, lb], [0.002, -0.002 + mult * sd], cands=[[la], [lb]])
        if spurious_holds(F["spurious"][3], *system(F["spurious"]))[0]:
            break
    # moved (not one of NAMES; the budget tests' long search, 180 nodes on C1): clean's lists with bearing 1 moved by 1.7
    # sqrt(S_ii) and its list cut down to its true landmark, so the first descent is not the winner
    off = alt(m)
    off[1] += 1.7 * float(np.sqrt(F["clean/var"][1, 0]))
    frame("moved", [a] * m, obs[:m], off, cands=[[obs[1]] if t == 1 else list(c) for t, c in enumerate(F["clean"][3])])
    frame("conflict", [a] * m, [obs[0]] + obs[:m - 1], [0.002, -0.002] + alt(m)[2:])
    p, z, om, c = F["conflict"]
    F["conflict"] = (p, z, om, [c[0], [c[0][0]] + [l for l in c[1] if l != c[0][0]][:2]] + c[2:])
    F["twin"] = (np.array([a, a], dtype=np.int32), np.full(2, pred(a, obs[0]) + 0.002), np.full(2, OMEGA), [[obs[0]], [obs[0]]])
    p, z, om, c = F["clean"]
    F["no_candidates"] = (p, z, om, [[] if b in (1, m - 1) else list(c[b]) for b in range(m)])
    F["empty"] = (np.zeros(0, dtype=np.int32), np.zeros(0), np.zeros(0), [])
    fo = observed(P, P.fixed)[:4]
    frame("fixed_pose", [P.fixed] * len(fo), fo, alt(len(fo)))
    a2 = max([p for p in free if p != a], key=lambda p: (len(observed(P, p)), -p))
    o2 = observed(P, a2)[:2]
    frame("two_poses", [a] * min(3, m) + [a2] * len(o2), obs[:min(3, m)] + o2, alt(min(3, m) + len(o2)))
    # full: 8 x 4, the true landmark first
    ring = (obs + others)[:8]
    nb, nc = min(8, len(ring)), min(4, len(ring))
    frame("full", [a] * nb, ring[:nb], alt(nb), cands=[[ring[(b + i) % len(ring)] for i in range(nc)] for b in range(nb)])
    # deep: 20 x 1 + 6 x 2
    world = obs + others
    n_two = 6 if len(world) >= 32 else min(2, len(world) // 4)
    n_one = 20 if len(world) >= 32 else max(0, min(len(world) - 2 * n_two, 20))
    deep = world[:n_one + n_two]
    spare = world[n_one + n_two:n_one + 2 * n_two]
    cands = [[l] for l in deep[:n_one]] + [[l, s] for l, s in zip(deep[n_one:], spare)]
    frame("deep", [a] * len(deep), deep, alt(len(deep)), cands=cands)
    return {k: v for k, v in F.items() if "/" not in k or k == "spurious/rho"}


NAMES = ("clean", "spurious", "conflict", "twin", "no_candidates", "empty", "fixed_pose", "two_poses", "full", "deep")


def frame_list(F, names=NAMES):
    return [F[n] for n in names]


def frame_slices(out, f):
    """(bearings, pairings) of frame f of a result"""
    fs, cs = out["frame_start"], out["cand_start"]
    return slice(fs[f], fs[f + 1]), slice(cs[fs[f]], cs[fs[f + 1]])


def same_frame(x, fx, y, fy, cov=True):
    """Frame fy of result y equals frame fx of result x, bit for bit."""
    bx, px = frame_slices(x, fx)
    by, py = frame_slices(y, fy)
    for k in ("assignment", "prefix_nis"):
        assert np.array_equal(x[k][bx], y[k][by]), (k, fx, fy)
    for k in ("n_paired", "joint_nis", "complete"):
        assert x[k][fx] == y[k][fy], (k, fx, fy)
    assert np.array_equal(x["innovation"][px], y["innovation"][py]), (fx, fy)
    if cov:
        assert np.array_equal(x["innovation_cov"][fx], y["innovation_cov"][fy]), (fx, fy)


def check_frame(out, f, cands, search_host=None, label=""):
    """Frame f of a result against the enumeration on the result's own S_all and e_all (at most BRUTE_LEAVES
    leaves), or against search_host(cands, S, e) (bos.jcbb_search_host with the bound off or a raised budget).
    Returns the enumeration (or None)."""
    b, p = frame_slices(out, f)
    S, e = out["innovation_cov"][f], out["innovation"][p]
    assert out["complete"][f] == 1, label
    if search_host is None:
        assert leaves(cands) <= BRUTE_LEAVES, label
        ref = brute_force(cands, S, e)
    else:
        ref = search_host(cands, S, e)
        assert ref["complete"] == 1, label
    assert np.array_equal(out["assignment"][b], ref["assignment"]), (label, out["assignment"][b], ref["assignment"])
    assert out["n_paired"][f] == ref["n_paired"], label
    assert out["joint_nis"][f] == ref["joint_nis"], label
    assert np.array_equal(out["prefix_nis"][b], ref["prefix_nis"]), label
    return ref if search_host is None else None


def winner_hypothesis(out, f, frame):
    """(pose, landmark, z, omega) of frame f's result as one hypothesis of the joint call, and its bearings"""
    b, _ = frame_slices(out, f)
    pose, z, om, _ = frame
    asg = out["assignment"][b]
    on = np.flatnonzero(asg >= 0)
    return (np.asarray(pose)[on], asg[on], np.asarray(z)[on], np.asarray(om)[on]), on


def all_pairings(frame):
    """(pose, landmark, z, omega) of a frame's all-pairings hypothesis"""
    pose, z, om, cands = frame
    n = [len(c) for c in cands]
    return (np.repeat(np.asarray(pose, dtype=np.int32), n), np.array([l for c in cands for l in c], dtype=np.int32),
            np.repeat(np.asarray(z, dtype=np.float64), n), np.repeat(np.asarray(om, dtype=np.float64), n))


def check_against_joint(out, frames, joint):
    """innovation and innovation_cov are the all-pairings hypotheses', joint_nis and prefix_nis at the paired
    bearings the winner's, bit for bit. joint(list of (pose, landmark, z, omega)) -> result of the joint call
    with cov."""
    hyps = [all_pairings(fr) for fr in frames]
    win = [winner_hypothesis(out, f, fr) for f, fr in enumerate(frames)]
    res = joint(hyps + [w[0] for w in win])
    n = len(frames)
    hs = res["hyp_start"]
    for f in range(n):
        b, p = frame_slices(out, f)
        assert np.array_equal(out["innovation"][p], res["innovation"][hs[f]:hs[f + 1]]), f
        assert np.array_equal(out["innovation_cov"][f], res["innovation_cov"][f]), f
        on = win[f][1]
        assert np.array_equal(out["prefix_nis"][b][on], res["prefix_nis"][hs[n + f]:hs[n + f + 1]]), f
        assert out["joint_nis"][f] == res["joint_nis"][n + f], f
        assert out["n_paired"][f] == len(on)


def close_frames(P, vals, F, names, out, tol, **plan):
    """The frames (of at most BRUTE_LEAVES leaves) whose winner, by the enumeration on the result's own system, does
    not beat the runner-up by count or by a NIS margin larger than joint_ref's NIS bound of the two hypotheses
    (2 tol (sum |x_i| s_i)^2 + 64 eps n kappa_2(S) nis each, s_i from the host's pair covariances at P's state): a
    second evaluation of the same system within tol may choose the other one. Prints every margin."""
    from edge_cov_ref import bearing_jacobians
    from helpers import EPS
    close = []
    for f, name in enumerate(names):
        if leaves(F[name][3]) > BRUTE_LEAVES:
            continue
        _, p = frame_slices(out, f)
        Sg, e = out["innovation_cov"][f], out["innovation"][p]
        ref = brute_force(F[name][3], Sg, e)
        if ref["runner_up"] is None or ref["runner_up"][0] < ref["n_paired"]:
            continue
        pose, lm, _, _ = all_pairings(F[name])
        pc = bos.plan_mf_pair_covariances(P, vals, pose, P.NP + lm, **plan)
        sd = np.sqrt(np.concatenate([np.diagonal(pc["cov_a"].reshape(-1, 3, 3), axis1=1, axis2=2),
                                     np.diagonal(pc["cov_b"][:, :4].reshape(-1, 2, 2), axis1=1, axis2=2)], axis=1))
        s = (np.abs(bearing_jacobians(P.pose_xyt[pose], P.lm_xy[lm])) * sd).sum(axis=1)
        bound = 0.0
        for q, nis in ((ref["pairings"], ref["joint_nis"]), (ref["runner_up_pairings"], ref["runner_up"][1])):
            Sq, eq = Sg[np.ix_(q, q)], e[q]
            x = np.linalg.solve(Sq, eq)
            bound += 2 * tol * (np.abs(x) * s[q]).sum() ** 2 + 64 * EPS * len(q) * np.linalg.cond(Sq) * nis
        margin = ref["runner_up"][1] - ref["joint_nis"]
        print(f"    {name}: NIS margin to the runner-up {margin:.3g}, bound {bound:.3g}")
        if not margin > bound:
            close.append(name)
    return close


def check_exact_rules(frames, run):
    """Two calls, a repeated frame, another order and company, a frame alone and one frame per batch: identical
    bits. run(frames, batch=0) -> result with cov."""
    n = len(frames)
    full = run(frames + [frames[0]])
    again = run(frames + [frames[0]])
    for f in range(n + 1):
        same_frame(full, f, again, f)
    same_frame(full, 0, full, n)
    order = list(reversed(range(n)))
    rev = run([frames[f] for f in order])
    for i, f in enumerate(order):
        same_frame(full, f, rev, i)
    for f in (0, n // 2, n - 1):
        same_frame(full, f, run([frames[f]]), 0)
    split = run(frames, batch=1)
    for f in range(n):
        same_frame(full, f, split, f)
    return full
