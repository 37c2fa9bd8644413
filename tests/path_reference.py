"""Waypoint paths: the NORMATIVE loop of include/pick_ik_amd.h (pikamd_solve_paths) over any solve_batch-shaped
callable -- the CPU oracle, or a handle's own solve_batch -- and the two fixture generators of the path tests."""
import numpy as np

NOT_ATTEMPTED = 0
PATH_JUMP = -1001
STATS_DTYPE = np.dtype([("cost_evals", "<i8"), ("generations", "<i4"), ("wipeouts", "<i4"), ("pool_erasures", "<i4"),
                        ("reserved", "<i4")])


def reference_paths(solve, goals, start, max_joint_step=None):
    """solve(goal [n]..., seed [n][dof]) -> (solution, status, cost, stats): a LOCAL-mode solve_batch whose search
    starts at the seed.  goals [P][W][7] or [P][W][n_tips][7], start [P][dof], max_joint_step [dof] or None.
    Returns (solution [P][W][dof], status [P][W], cost [P][W], stats [P][W], reached [P])."""
    goals = np.asarray(goals, dtype=np.float64)
    seed = np.array(start, dtype=np.float64)
    P, W = goals.shape[:2]
    dof = seed.shape[1]
    lim = None if max_joint_step is None else np.asarray(max_joint_step, dtype=np.float64)
    solution = np.empty((P, W, dof))
    status = np.empty((P, W), dtype=np.int32)
    cost = np.empty((P, W))
    stats = np.zeros((P, W), dtype=STATS_DTYPE)
    reached = np.zeros(P, dtype=np.int32)
    held = np.ones(P, dtype=bool)
    for k in range(W):
        idx = np.nonzero(held)[0]
        behind = np.nonzero(~held)[0]
        solution[behind, k] = seed[behind]
        status[behind, k] = NOT_ATTEMPTED
        cost[behind, k] = 0.0  # (stats: zero already)
        if len(idx) == 0:
            continue
        sol, st, c, stt = solve(goals[idx, k], seed[idx])
        for n, p in enumerate(idx):
            jump = False
            if st[n] > 0 and lim is not None:
                with np.errstate(invalid="ignore"):
                    jump = bool(np.any((lim > 0.0) & (np.abs(sol[n] - seed[p]) > lim)))
            if st[n] > 0 and not jump:
                solution[p, k] = sol[n]
                status[p, k] = st[n]
                seed[p] = sol[n]
                reached[p] += 1
            else:
                solution[p, k] = seed[p]
                status[p, k] = PATH_JUMP if jump else st[n]
                held[p] = False
            cost[p, k] = c[n]
            for f in STATS_DTYPE.names:
                stats[f][p, k] = stt[f][n]
    return solution, status, cost, stats, reached


def path_counts(status):
    """(complete paths, paths stopped strictly inside, paths stopped at waypoint 0, paths stopped by a jump)"""
    status = np.asarray(status)
    held = status > 0
    complete = held.all(axis=1)
    at0 = ~held[:, 0]
    inside = ~complete & ~at0
    return int(complete.sum()), int(inside.sum()), int(at0.sum()), int((status == PATH_JUMP).any(axis=1).sum())


def _spans(chain, cap=None):
    mid = 0.5 * (np.asarray(chain.qmin) + np.asarray(chain.qmax))
    half = 0.5 * (np.asarray(chain.qmax) - np.asarray(chain.qmin))
    return mid, (half if cap is None else np.minimum(half, cap))


def straight_lines(chain, fk, P=64, W=32, L=0.3):
    """Rigid Cartesian straight lines (one tip): the pose of a random configuration translated by L * (k + 1) / W
    along a random direction, orientation kept.  Returns (goals [P][W][7], start [P][dof])."""
    rng = np.random.default_rng(1)
    mid, half = _spans(chain)
    q0 = mid + 0.6 * half * rng.uniform(-1.0, 1.0, size=(P, chain.dof))
    d = rng.normal(size=(P, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    pose = np.asarray(fk(q0)).reshape(P, 7)
    goals = np.repeat(pose[:, None, :], W, axis=1)
    goals[:, :, :3] += (L * (np.arange(W) + 1.0) / W)[None, :, None] * d[:, None, :]
    return np.ascontiguousarray(goals), q0


def joint_lines(chain, fk, P=32, W=16, fixed=None):
    """Poses along straight lines in JOINT space (reachable by construction, any number of tips): waypoint k is
    fk(q0 + dq * (k + 1) / W), |dq| = 0.5.  fixed = (variables, values): variables that do not move and take these
    values in q0 (a floating base).  Returns (goals [P][W][7] or [P][W][n_tips][7], start [P][dof])."""
    rng = np.random.default_rng(2)
    mid, half = _spans(chain, cap=1.0)
    q0 = mid + 0.5 * half * rng.uniform(-1.0, 1.0, size=(P, chain.dof))
    dq = rng.normal(size=(P, chain.dof))
    if fixed is not None:
        q0[:, fixed[0]] = np.asarray(fixed[1], dtype=np.float64)
        dq[:, fixed[0]] = 0.0
    dq *= 0.5 / np.linalg.norm(dq, axis=1, keepdims=True)
    q = q0[:, None, :] + dq[:, None, :] * ((np.arange(W) + 1.0) / W)[None, :, None]
    g = np.asarray(fk(q.reshape(P * W, chain.dof)))
    return np.ascontiguousarray(g.reshape((P, W) + g.shape[1:])), q0


def host_loop(solver, params, goals, start):
    """What a caller writes today: W dependent local-mode solve_batch calls, each from the previous answers, the paths
    that stopped taken out of the batch by hand (no step limit).  Returns reached [P]."""
    P, W = goals.shape[:2]
    seed = np.array(start, dtype=np.float64)
    held = np.arange(P)
    reached = np.zeros(P, dtype=np.int32)
    for k in range(W):
        sol, st, _, _ = solver.solve_batch(params, goals[held, k], seed[held])
        ok = st > 0
        held = held[ok]
        seed[held] = sol[ok]
        reached[held] += 1
        if len(held) == 0:
            break
    return reached


def time_paths_against_loop(solver, params, goals, start, reps=21):
    """Wall-clock seconds of solve_paths and of host_loop on the same paths: both warmed, then alternated `reps`
    times, a host clock around calls that end synchronised.  Returns (median paths, median loop, all paths, all loop)."""
    import time
    for _ in range(2):
        r = solver.solve_paths(params, goals, start)[4]
        np.testing.assert_array_equal(r, host_loop(solver, params, goals, start))
    tp, tl = [], []
    for _ in range(reps):
        t0 = time.perf_counter()
        solver.solve_paths(params, goals, start)
        t1 = time.perf_counter()
        host_loop(solver, params, goals, start)
        t2 = time.perf_counter()
        tp.append(t1 - t0)
        tl.append(t2 - t1)
    return float(np.median(tp)), float(np.median(tl)), tp, tl
