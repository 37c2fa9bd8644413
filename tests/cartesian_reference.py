"""computeCartesianPath in one call: the NORMATIVE loop of include/pick_ik_amd.h (pikamd_cartesian_paths) over any
solve_batch-shaped callable -- the CPU oracle, or a handle's own solve_batch --, built on path_reference.reference_paths,
and the fixture generators of the Cartesian tests.  The poses and step counts come from the caller (the library's host
function pikamd_interpolate_poses applied to a forward kinematics): the loop itself is the solve side."""
import numpy as np

from tests import path_reference as PR

NOT_ATTEMPTED = 0
PATH_JUMP = -1001
PATH_RELATIVE_JUMP = -1003
NAMES = ("solution", "status", "cost", "stats", "reached", "steps", "fraction")


def relative_jump(traj, factor):
    """MoveIt's checkRelativeJointSpaceJump over traj [r + 1][dof]: the first i whose step is further than factor times
    the mean step, or None.  Every sum from 0.0, ascending, every operation rounded on its own."""
    r = len(traj) - 1
    dist = []
    for i in range(r):
        d = np.float64(0.0)
        for j in range(traj.shape[1]):
            d = d + np.abs(traj[i + 1][j] - traj[i][j])
        dist.append(d)
    total = np.float64(0.0)
    for d in dist:
        total = total + d
    thres = np.float64(factor) * (total / np.float64(r))
    for i, d in enumerate(dist):
        if d > thres:
            return i
    return None


def reference_cartesian(solve, goals, steps, start, jump_factor=0.0, max_joint_step=None):
    """solve: as path_reference.reference_paths takes it.  goals [P][W][7] and steps [P]: what pikamd_interpolate_poses
    gives for the poses of `start`; start [P][dof].  Returns (solution [P][W][dof], status [P][W], cost [P][W],
    stats [P][W], reached [P], steps [P], fraction [P]) and, beside them, held [P]: the waypoints the solve held before
    the relative test (what tells a relative stop on an otherwise complete path)."""
    goals = np.asarray(goals, dtype=np.float64)
    start = np.asarray(start, dtype=np.float64)
    steps = np.asarray(steps, dtype=np.int32)
    P, W = goals.shape[:2]
    dof = start.shape[1]
    solution = np.empty((P, W, dof))
    status = np.zeros((P, W), dtype=np.int32)
    cost = np.zeros((P, W))
    stats = np.zeros((P, W), dtype=PR.STATS_DTYPE)
    reached = np.zeros(P, dtype=np.int32)
    fraction = np.zeros(P)
    held = np.zeros(P, dtype=np.int32)
    solution[:] = start[:, None, :]  # (a path with n > W: every row the start, not attempted)
    # (paths with the same step count are solved together: a path's rows do not depend on its neighbours)
    for n in sorted(set(int(v) for v in steps if v <= W)):
        idx = np.nonzero(steps == n)[0]
        sol, st, c, stt, r = PR.reference_paths(solve, goals[idx, :n], start[idx], max_joint_step)
        solution[idx, :n] = sol
        status[idx, :n] = st
        cost[idx, :n] = c
        stats[idx, :n] = stt
        solution[idx, n:] = sol[:, n - 1:n]
        held[idx] = r
        for m, p in enumerate(idx):
            rr = int(r[m])
            fraction[p] = np.float64(rr) / np.float64(n)
            if jump_factor > 0.0 and rr >= 1:
                traj = np.concatenate([start[p][None], solution[p, :rr]])
                i = relative_jump(traj, jump_factor)
                if i is not None:
                    fraction[p] = fraction[p] * (np.float64(i + 1) / np.float64(rr + 1))
                    solution[p, i:] = traj[i]
                    status[p, i] = PATH_RELATIVE_JUMP
                    status[p, i + 1:] = NOT_ATTEMPTED
                    cost[p, i + 1:] = 0.0
                    stats[p, i + 1:] = np.zeros((), dtype=PR.STATS_DTYPE)
                    rr = i
            reached[p] = rr
    return (solution, status, cost, stats, reached, steps.copy(), fraction), held


def classes(result, held, W):
    """how many paths ended in each way: (complete, stopped by the solver, refused absolute jump, refused relative jump,
    too long, relative stops on an otherwise complete path)"""
    solution, status, cost, stats, reached, steps, fraction = result
    long_ = steps > W
    relative = (status == PATH_RELATIVE_JUMP).any(axis=1)
    absolute = (status == PATH_JUMP).any(axis=1) & ~relative
    complete = ~long_ & (reached == steps)
    solver = ~long_ & ~relative & ~absolute & ~complete
    return (int(complete.sum()), int(solver.sum()), int(absolute.sum()), int(relative.sum()), int(long_.sum()),
            int((relative & (held == steps)).sum()))


def _starts(chain, rng, P):
    mid = 0.5 * (np.asarray(chain.qmin) + np.asarray(chain.qmax))
    half = 0.5 * (np.asarray(chain.qmax) - np.asarray(chain.qmin))
    return mid + 0.6 * half * rng.uniform(-1.0, 1.0, size=(P, chain.dof))


#: the parameters of the fixture "offsets": (frame OFFSET = 2, min_steps, max_translation, max_rotation, jump_factor)
OFFSETS = dict(frame=2, min_steps=3, max_translation=0.04, max_rotation=0.0, jump_factor=1.12)


def offsets(chain, P=70, seed=7):
    """The fixture "panda offsets" (any chain): starts mid + 0.6 half U(-1, 1), targets in the OFFSET frame -- unit
    directions times lengths U(0.02, 0.6).  Returns (start [P][dof], target [P][7]); W = 12 and OFFSETS go with it."""
    rng = np.random.default_rng(seed)
    start = _starts(chain, rng, P)
    d = rng.normal(size=(P, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    target = np.zeros((P, 7))
    target[:, :3] = d * rng.uniform(0.02, 0.6, size=(P, 1))
    target[:, 3] = 1.0
    return start, target


def _quat_mul(a, b):
    aw, ax, ay, az = a.T
    bw, bx, by, bz = b.T
    return np.stack([aw * bw - ax * bx - ay * by - az * bz, aw * bx + ax * bw + ay * bz - az * by,
                     aw * by - ax * bz + ay * bw + az * bx, aw * bz + ax * by - ay * bx + az * bw], axis=1)


def _rotate(q, v):
    """R(q) v for unit quaternions [n][4] (w x y z)"""
    p = np.concatenate([np.zeros((len(v), 1)), v], axis=1)
    conj = q * np.array([1.0, -1.0, -1.0, -1.0])
    return _quat_mul(_quat_mul(q, p), conj)[:, 1:]


def rotating(chain, fk, frame, P=20, distance=0.5, seed=11):
    """Targets that rotate: the pose of a configuration at joint distance `distance` from the start, as a pose in the
    base frame (frame 0) or relative to the start tip frame (frame 1).  Returns (start [P][dof], target [P][7])."""
    rng = np.random.default_rng(seed)
    start = _starts(chain, rng, P)
    dq = rng.normal(size=(P, chain.dof))
    dq *= distance / np.linalg.norm(dq, axis=1, keepdims=True)
    a = np.asarray(fk(start)).reshape(P, 7)
    b = np.asarray(fk(start + dq)).reshape(P, 7)
    if frame == 0:
        return start, b
    conj = a[:, 3:] * np.array([1.0, -1.0, -1.0, -1.0])
    target = np.empty((P, 7))
    target[:, :3] = _rotate(conj, b[:, :3] - a[:, :3])
    target[:, 3:] = _quat_mul(conj, b[:, 3:])
    return start, target


def time_cartesian_against_padded(solver, params, cartesian, start, target, W, interpolate, reps=11):
    """Wall-clock seconds of cartesian_paths and of what a caller writes without it -- fk, the host interpolation,
    solve_paths on every path padded to W --, both warmed, then alternated `reps` times, a host clock around calls
    that end synchronised.  Returns (median call, median loop)."""
    import time

    def loop():
        goals, _ = interpolate(cartesian, solver.fk(start), target, W)
        return solver.solve_paths(params, goals, start)

    for _ in range(2):
        solver.cartesian_paths(params, cartesian, start, target, W)
        loop()
    tc, tl = [], []
    for _ in range(reps):
        t0 = time.perf_counter()
        solver.cartesian_paths(params, cartesian, start, target, W)
        t1 = time.perf_counter()
        loop()
        t2 = time.perf_counter()
        tc.append(t1 - t0)
        tl.append(t2 - t1)
    return float(np.median(tc)), float(np.median(tl))
