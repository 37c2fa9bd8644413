"""computeCartesianPath through waypoints: the NORMATIVE loop of include/pick_ik_amd.h (pikamd_cartesian_waypoints) over
any solve_batch-shaped callable -- the CPU oracle, or a handle's own solve_batch --, built on
cartesian_reference.reference_cartesian (one segment of one path is one pikamd_cartesian_paths call with P = 1; the
paths whose segment has the same room are handed over together, which changes no row: a path's rows do not depend on
its neighbours), and the fixture generators of the waypoint-list tests."""
import numpy as np

from tests import cartesian_reference as CR
from tests import path_reference as PR

NAMES = CR.NAMES + ("goals", "segment_steps")
INT32_MAX = 2**31 - 1
# how a path ended before the relative test
NONE, COMPLETE, SOLVER, ABSOLUTE, NO_FIT = 0, 1, 2, 3, 4


def reference_polyline(solve, fk, interpolate, cartesian, start, targets, W, n_targets=None, max_joint_step=None):
    """solve: as path_reference.reference_paths takes it; fk: configurations [n][dof] -> poses [n][7];
    interpolate(c, start_pose, target, W) -> (goals, steps): pikamd_interpolate_poses of the library under test.
    start [P][dof], targets [P][S][7].  Returns the nine arrays (solution, status, cost, stats, reached, steps, fraction,
    goals, segment_steps) and, beside them, what the class counts read: kind [P] (how the path ended before the
    relative test), seg [P] (the segment it ended in), held [P], frac [P] (the fraction before the relative test),
    no_room [P] (a target was left when every row was taken), moved [P] (boundaries at which the pose of the state
    differs in bits from the previous segment's last pose)."""
    start = np.asarray(start, dtype=np.float64)
    targets = np.asarray(targets, dtype=np.float64)
    P, S = targets.shape[:2]
    dof = start.shape[1]
    c1 = type(cartesian)(frame=cartesian.frame, min_steps=cartesian.min_steps, max_translation=cartesian.max_translation,
                         max_rotation=cartesian.max_rotation, jump_factor=0.0)
    sp = np.full(P, S, dtype=np.int64) if n_targets is None else np.clip(np.asarray(n_targets, dtype=np.int64), 0, S)
    solution = np.empty((P, W, dof))
    solution[:] = start[:, None, :]
    status = np.zeros((P, W), dtype=np.int32)
    cost = np.zeros((P, W))
    stats = np.zeros((P, W), dtype=PR.STATS_DTYPE)
    goals = np.zeros((P, W, 7))
    segment_steps = np.zeros((P, S), dtype=np.int32)
    cur = start.copy()
    off = np.zeros(P, dtype=np.int64)
    held = np.zeros(P, dtype=np.int64)
    need = np.zeros(P, dtype=np.int64)
    frac = np.zeros(P)
    open_ = sp > 0
    kind = np.where(open_, COMPLETE, NONE)
    seg = np.zeros(P, dtype=np.int64)
    no_room = np.zeros(P, dtype=bool)
    moved = np.zeros(P, dtype=np.int64)
    zero = np.zeros((), dtype=PR.STATS_DTYPE)
    for i in range(S):
        todo = np.nonzero(open_ & (i < sp))[0]
        if len(todo) == 0:
            break
        pose = np.asarray(fk(cur[todo])).reshape(len(todo), 7)
        for room in sorted(set(int(v) for v in W - off[todo])):
            sel = np.nonzero(W - off[todo] == room)[0]
            idx = todo[sel]
            if room == 0:
                g, n = interpolate(c1, pose[sel], targets[idx, i], 1)
                out = None
            else:
                g, n = interpolate(c1, pose[sel], targets[idx, i], room)
                out, _ = CR.reference_cartesian(solve, g, n, cur[idx], 0.0, max_joint_step)
            for m, p in enumerate(idx):
                o, n_i = int(off[p]), int(n[m])
                seg[p] = i
                segment_steps[p, i] = n_i
                need[p] = min(o + n_i, INT32_MAX)
                if i > 0 and pose[sel][m].tobytes() != goals[p, o - 1].tobytes():
                    moved[p] += 1
                if room > 0:
                    goals[p, o:] = g[m]
                else:
                    no_room[p] = True
                if n_i > room:  # did not fit: the fraction stays
                    solution[p, o:] = cur[p]
                    status[p, o:] = CR.NOT_ATTEMPTED
                    cost[p, o:] = 0.0
                    stats[p, o:] = zero
                    open_[p] = False
                    kind[p] = NO_FIT
                    continue
                solution[p, o:], status[p, o:], cost[p, o:], stats[p, o:] = out[0][m], out[1][m], out[2][m], out[3][m]
                r = int(out[4][m])
                held[p] = o + r
                if r == n_i:
                    frac[p] = np.float64(i + 1) / np.float64(sp[p])
                    cur[p] = solution[p, o + n_i - 1]
                    off[p] += n_i
                else:
                    frac[p] = np.float64(i) / np.float64(sp[p]) + (np.float64(r) / np.float64(n_i)) / np.float64(sp[p])
                    open_[p] = False
                    kind[p] = ABSOLUTE if status[p, o + r] == CR.PATH_JUMP else SOLVER
    reached = np.zeros(P, dtype=np.int32)
    fraction = frac.copy()
    for p in range(P):
        r = int(held[p])
        if cartesian.jump_factor > 0.0 and r >= 1:
            traj = np.concatenate([start[p][None], solution[p, :r]])
            i = CR.relative_jump(traj, cartesian.jump_factor)
            if i is not None:
                fraction[p] = fraction[p] * (np.float64(i + 1) / np.float64(r + 1))
                solution[p, i:] = traj[i]
                status[p, i] = CR.PATH_RELATIVE_JUMP
                status[p, i + 1:] = CR.NOT_ATTEMPTED
                cost[p, i + 1:] = 0.0
                stats[p, i + 1:] = zero
                r = i
        reached[p] = r
    info = dict(kind=kind, seg=seg, held=held.astype(np.int32), frac=frac, no_room=no_room, moved=moved, n_targets=sp)
    return (solution, status, cost, stats, reached, need.astype(np.int32), fraction, goals, segment_steps), info


def classes(result, info, W, S):
    """how many paths ended in each way.  complete: every segment held and no relative stop; solver_later /
    absolute_later: the walk stopped in a segment behind the first (a relative stop may cut such a path further in
    front); relative_later: a relative stop whose row lies behind segment 0; relative_on_complete: a relative stop on a
    path every segment of which held; no_fit_first / no_fit_later: a segment had more steps than rows were left;
    fewer_targets: n_targets < S; no_room: a target was left when every row was taken; moved_boundary: paths with a
    boundary at which the pose of the state differs in bits from the previous segment's last pose; different_steps: the
    distinct values of steps among the paths that fitted"""
    solution, status, cost, stats, reached, steps, fraction, goals, segment_steps = result
    kind, seg, held = info["kind"], info["seg"], info["held"]
    relative = (status == CR.PATH_RELATIVE_JUMP).any(axis=1)
    later = reached >= segment_steps[:, 0]  # (a relative stop: its row lies behind segment 0)
    walked = steps[(steps <= W) & (steps > 0)]
    return dict(
        complete=int(((kind == COMPLETE) & ~relative).sum()),
        solver_later=int(((kind == SOLVER) & (seg >= 1)).sum()),
        absolute_later=int(((kind == ABSOLUTE) & (seg >= 1)).sum()),
        relative_later=int((relative & later).sum()),
        relative_on_complete=int((relative & (kind == COMPLETE)).sum()),
        no_fit_first=int(((kind == NO_FIT) & (seg == 0)).sum()),
        no_fit_later=int(((kind == NO_FIT) & (seg >= 1)).sum()),
        fewer_targets=int((info["n_targets"] < S).sum()),
        no_room=int(info["no_room"].sum()),
        moved_boundary=int((info["moved"] > 0).sum()),
        different_steps=len(set(int(v) for v in walked)),
    )


#: what the table asks of the fixture "panda polylines" without a step limit; with the limit, absolute_later as well
MINIMA = dict(complete=4, solver_later=2, relative_later=1, relative_on_complete=1, no_fit_first=1, no_fit_later=2,
              fewer_targets=4, no_room=1, moved_boundary=1, different_steps=4)
MINIMA_LIMITED = dict(absolute_later=2)

#: the parameters of the fixture "panda polylines" (frame OFFSET = 2); S = 3 and W = 16 go with it
POLYLINES = dict(frame=2, min_steps=2, max_translation=0.04, max_rotation=0.0, jump_factor=1.1)
S_POLYLINES, W_POLYLINES = 3, 16


def polylines(chain, P=70, S=S_POLYLINES, seed=5):
    """The fixture "panda polylines" (any chain): starts as cartesian_reference.offsets has them, S offsets per path --
    unit directions times lengths U(0.02, 0.3) --, n_targets mixed over 1..S.  Some paths are made for a class:
    path 0 has a first segment too long for 16 rows, paths 1 and 2 two segments of eight steps and a target left (no
    room), paths 3..14 go on in one direction (they leave the workspace in a later segment).  Returns (start [P][dof],
    targets [P][S][7], n_targets [P])."""
    rng = np.random.default_rng(seed)
    start = CR._starts(chain, rng, P)
    d = rng.normal(size=(P, S, 3))
    d /= np.linalg.norm(d, axis=2, keepdims=True)
    length = rng.uniform(0.02, 0.3, size=(P, S, 1))
    n_targets = rng.integers(1, S + 1, size=P).astype(np.int32)
    if P >= 15 and S >= 3:
        length[0, 0] = 0.7
        n_targets[0] = S
        length[1:3, :2] = 0.3
        d[1:3, 1] = -d[1:3, 0]  # (there and back: reachable)
        n_targets[1:3] = S
        d[3:15, 1:] = d[3:15, :1]
        length[3:15] = 0.29
        n_targets[3:15] = S
    targets = np.zeros((P, S, 7))
    targets[:, :, :3] = d * length
    targets[:, :, 3] = 1.0
    return start, targets, n_targets


def _relative(a, b):
    """the pose b [n][7] relative to the tip frame a [n][7]: a * result = b"""
    conj = a[:, 3:] * np.array([1.0, -1.0, -1.0, -1.0])
    out = np.empty_like(b)
    out[:, :3] = CR._rotate(conj, b[:, :3] - a[:, :3])
    out[:, 3:] = CR._quat_mul(conj, b[:, 3:])
    return out


def turning(chain, fk, P=20, S=2, distance=0.35, seed=13):
    """The fixture "turning": S targets in the TIP frame -- the poses of configurations at joint distance `distance`
    from one another, each relative to the pose before it (the state a segment ends in is near that pose, not on it).
    Returns (start [P][dof], targets [P][S][7])."""
    rng = np.random.default_rng(seed)
    q = CR._starts(chain, rng, P)
    start = q.copy()
    pose = np.asarray(fk(q)).reshape(P, 7)
    targets = np.empty((P, S, 7))
    for i in range(S):
        dq = rng.normal(size=(P, chain.dof))
        dq *= distance / np.linalg.norm(dq, axis=1, keepdims=True)
        q = q + dq
        nxt = np.asarray(fk(q)).reshape(P, 7)
        targets[:, i] = _relative(pose, nxt)
        pose = nxt
    return start, targets


def time_waypoints_against_host_loop(solver, params, cartesian, start, targets, W, n_targets=None, reps=11):
    """Wall-clock seconds of cartesian_waypoints and of what a caller writes without it: S cartesian_paths calls, the
    host picking and repacking the complete paths between them (one call per segment, at the largest room: a lower
    bound for the caller's loop), the stitched relative test in numpy.  Both warmed, then alternated `reps` times, a host clock around calls that end synchronised.  Returns (median call, median loop)."""
    import time

    P, S = targets.shape[:2]
    sp = np.full(P, S) if n_targets is None else np.clip(n_targets, 0, S)
    c1 = type(cartesian)(frame=cartesian.frame, min_steps=cartesian.min_steps,
                         max_translation=cartesian.max_translation, max_rotation=cartesian.max_rotation, jump_factor=0.0)

    def loop():
        rows = np.tile(start[:, None, :], (1, W, 1))
        status, cost = np.zeros((P, W), dtype=np.int32), np.zeros((P, W))
        stats, goals = np.zeros((P, W), dtype=PR.STATS_DTYPE), np.zeros((P, W, 7))
        cur, off, alive = start.copy(), np.zeros(P, dtype=np.int64), sp > 0
        held, frac = np.zeros(P, dtype=np.int64), np.zeros(P)
        for i in range(S):
            idx = np.nonzero(alive & (i < sp) & (off < W))[0]
            if len(idx) == 0:
                break
            # (ONE call per segment, at the largest room of the paths still open -- a path's rows do not depend on W as
            # long as its segment fits --; a call per distinct offset would be more calls: this loop is a lower bound
            # for what a caller writes)
            room = int(W - off[idx].min())
            sol, st, c, stt, reached, steps, _, g = solver.cartesian_paths(params, c1, cur[idx], targets[idx, i], room, None)
            for m, p in enumerate(idx):
                n, r, o = int(steps[m]), int(reached[m]), int(off[p])
                if n > W - o:
                    alive[p] = False
                    continue
                k = min(n, r + 1)  # (the rows solved: the held ones and the refused one)
                rows[p, o:o + n], goals[p, o:o + n] = sol[m, :n], g[m, :n]
                status[p, o:o + k], cost[p, o:o + k], stats[p, o:o + k] = st[m, :k], c[m, :k], stt[m, :k]
                rows[p, o + n:] = sol[m, n - 1]
                held[p] = o + r
                if r == n:
                    cur[p], off[p], frac[p] = sol[m, n - 1], o + n, (i + 1) / sp[p]
                else:
                    alive[p], frac[p] = False, (i + r / n) / sp[p]
        reached = held.copy()
        if cartesian.jump_factor > 0.0:
            for p in range(P):
                r = int(held[p])
                if r >= 1:
                    traj = np.concatenate([start[p][None], rows[p, :r]])
                    dist = np.abs(np.diff(traj, axis=0)).sum(axis=1)
                    over = np.nonzero(dist > cartesian.jump_factor * dist.mean())[0]
                    if len(over):
                        j = int(over[0])
                        frac[p] *= (j + 1) / (r + 1)
                        rows[p, j:] = traj[j]
                        status[p, j], status[p, j + 1:], cost[p, j + 1:] = CR.PATH_RELATIVE_JUMP, CR.NOT_ATTEMPTED, 0.0
                        stats[p, j + 1:] = np.zeros((), dtype=PR.STATS_DTYPE)
                        reached[p] = j
        return rows, status, cost, stats, reached, frac, goals

    for _ in range(2):
        solver.cartesian_waypoints(params, cartesian, start, targets, W, n_targets)
        loop()
    tc, tl = [], []
    for _ in range(reps):
        t0 = time.perf_counter()
        solver.cartesian_waypoints(params, cartesian, start, targets, W, n_targets)
        t1 = time.perf_counter()
        loop()
        t2 = time.perf_counter()
        tc.append(t1 - t0)
        tl.append(t2 - t1)
    return float(np.median(tc)), float(np.median(tl))
