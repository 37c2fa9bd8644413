"""Cartesian paths from a pose: the NORMATIVE loop of include/pick_ik_amd.h (pikamd_search_paths) over any
solve_batch-shaped callable -- the CPU oracle, or a handle's own solve_batch --, composed from the restart states of
tests/search_reference.py and the waypoint loop of tests/path_reference.py; the classes a fixture must reach; the
fixtures of the tests; and the loop a caller writes today."""
import dataclasses

import numpy as np

from pick_ik_amd import robots
from tests import path_reference as PR
from tests import search_reference as SR

STATS_DTYPE = SR.STATS_DTYPE
NAMES = ("solution", "status", "cost", "stats", "reached", "attempts", "totals")
CLASSES = ("complete at attempt 0", "complete later", "never complete, best > 0", "never complete, kept attempt later",
           "never complete, best == 0", "stopped by a jump")


@dataclasses.dataclass
class Trace:
    """what the loop did beyond its outputs: reached_a of every attempt a path ran (-1: not run), the attempt whose
    rows were kept, whether any attempt of the path was stopped by a refused jump, and the stats rows of every attempt
    as (paths that ran it, their rows [n][W]) -- what totals must be the sum of"""
    reached: np.ndarray  # [P][K]
    kept: np.ndarray     # [P]
    jumped: np.ndarray   # [P] bool
    attempt_stats: list


def reference_search_paths(solve, chain, goals, seed, max_attempts, max_joint_step=None, rng_seed=0, problem_offset=0,
                           initial_guess=None, trace=False):
    """solve(goal [n]..., seed [n][dof], initial_guess [n][dof]) -> (solution, status, cost, stats): a LOCAL-mode
    solve_batch.  goals [P][W][7] or [P][W][n_tips][7], seed [P][dof].  Returns (solution [P][W][dof], status [P][W],
    cost [P][W], stats [P][W], reached [P], attempts [P], totals [P]) and, with trace, a Trace behind them."""
    goals = np.asarray(goals, dtype=np.float64)
    seed = np.asarray(seed, dtype=np.float64)
    P, W = goals.shape[:2]
    dof, K = chain.dof, max_attempts
    table = SR.starts(chain, seed, K, rng_seed, problem_offset, initial_guess)  # init[p] in front of every attempt
    solution = np.empty((P, W, dof))
    status = np.empty((P, W), dtype=np.int32)
    cost = np.empty((P, W))
    stats = np.zeros((P, W), dtype=STATS_DTYPE)
    totals = np.zeros(P, dtype=STATS_DTYPE)
    attempts = np.zeros(P, dtype=np.int32)
    best = np.full(P, -1, dtype=np.int32)
    tr = Trace(np.full((P, K), -1, dtype=np.int32), np.zeros(P, dtype=np.int32), np.zeros(P, dtype=bool), [])
    is_open = np.ones(P, dtype=bool)
    for a in range(K):
        idx = np.nonzero(is_open)[0]
        if len(idx) == 0:
            break
        n = len(idx)
        sol0, st0, c0, stats0 = solve(goals[idx, 0], seed[idx], table[idx, a])
        ok = st0 > 0
        rows_sol = np.repeat(seed[idx][:, None, :], W, axis=1)       # rows 1.. of a failed waypoint 0: the seed,
        rows_st = np.full((n, W), PR.NOT_ATTEMPTED, dtype=np.int32)   # not attempted, cost 0, no statistics
        rows_cost = np.zeros((n, W))
        rows_stats = np.zeros((n, W), dtype=STATS_DTYPE)
        rows_sol[:, 0] = np.where(ok[:, None], sol0, seed[idx])       # (what the call returned: no joint-step test)
        rows_st[:, 0] = st0
        rows_cost[:, 0] = c0
        rows_stats[:, 0] = stats0
        reached_a = np.where(ok, 1, 0).astype(np.int32)
        tr.attempt_stats.append((idx, rows_stats))
        if W > 1 and ok.any():
            psol, pst, pcost, pstats, preached = PR.reference_paths(lambda g, sd: solve(g, sd, sd), goals[idx[ok], 1:],
                                                                    sol0[ok], max_joint_step)
            rows_sol[ok, 1:], rows_st[ok, 1:], rows_cost[ok, 1:], rows_stats[ok, 1:] = psol, pst, pcost, pstats
            reached_a[ok] += preached
        for m, p in enumerate(idx):
            for f in STATS_DTYPE.names:
                totals[f][p] += rows_stats[f][m].sum()
            attempts[p] = a + 1
            tr.reached[p, a] = reached_a[m]
            tr.jumped[p] |= bool((rows_st[m] == PR.PATH_JUMP).any())
            if reached_a[m] > best[p]:  # (first among equals wins)
                solution[p], status[p], cost[p], stats[p] = rows_sol[m], rows_st[m], rows_cost[m], rows_stats[m]
                best[p] = reached_a[m]
                tr.kept[p] = a
            if reached_a[m] == W:
                is_open[p] = False
    out = (solution, status, cost, stats, best.copy(), attempts, totals)
    return out + (tr,) if trace else out


def counts(out, tr):
    """paths per class, in the order of CLASSES"""
    W = out[1].shape[1]
    reached, attempts = out[4], out[5]
    done = reached == W
    return (int((done & (attempts == 1)).sum()), int((done & (attempts > 1)).sum()), int((~done & (reached > 0)).sum()),
            int((~done & (tr.kept > 0)).sum()), int((~done & (reached == 0)).sum()), int(tr.jumped.sum()))


def assert_classes(case, c, what=""):
    """every class the case claims is non-empty; a case without a step limit has no jump"""
    claims, limit = CASES[case][8], CASES[case][7]
    assert all(c[k] >= 1 for k in claims), (case, what, dict(zip(CLASSES, c)))
    assert limit is not None or c[5] == 0, (case, what, dict(zip(CLASSES, c)))
    assert c[0] + c[1] + c[2] + c[4] == CASES[case][3], (case, what, c)


def _mid(chain):
    return 0.5 * (np.asarray(chain.qmin) + np.asarray(chain.qmax))


#: rng_seed of the fixture tests
RNG_SEED = 1
#: name -> (chain, "straight" / "joint" lines, home pose or None = the middle of the limits, P, W, L (straight lines),
#: max_attempts, step limit of every variable or None, the classes of CLASSES the case claims to reach).  The seed of
#: every path is the home pose, not the line's own start.  Every case reaches the classes it claims under both oracle
#: math modes (tests/test_startpath_cpu.py asserts it); only a case without a step limit may leave the jumps out.  A
#: descent of the two-tip chain from a random configuration rarely solves waypoint 0: that case has one path that is
#: completed by a later attempt and none whose kept attempt is a later one.
EVERY_CLASS = (0, 1, 2, 3, 4, 5)
CASES = {
    "panda": (robots.panda, "straight", robots.PANDA_HOME, 48, 6, 0.3, 6, 0.15, EVERY_CLASS),
    "ur5": (robots.ur5, "straight", None, 48, 6, 0.3, 6, 0.15, EVERY_CLASS),
    "panda_no_step_limit": (robots.panda, "straight", robots.PANDA_HOME, 48, 6, 0.3, 6, None, (0, 1, 2, 3, 4)),
    "torso_dual_arm": (robots.torso_dual_arm, "joint", None, 64, 4, None, 8, None, (0, 1, 2, 4)),
    "panda_unbounded": (SR.panda_unbounded, "straight", robots.PANDA_HOME, 48, 6, 0.3, 6, 0.15, EVERY_CLASS),
}


def fixture(case, fk_of):
    """(chain, goals [P][W]..., seed [P][dof], max_attempts, max_joint_step [dof] or None) of one case.
    fk_of(chain) -> fk(q [n][dof])."""
    make, kind, home, P, W, L, K, limit, _ = CASES[case]
    ch = make()
    fk = fk_of(ch)
    goals, _ = PR.straight_lines(ch, fk, P=P, W=W, L=L) if kind == "straight" else PR.joint_lines(ch, fk, P=P, W=W)
    home = _mid(ch) if home is None else np.asarray(home, dtype=np.float64)
    seed = np.ascontiguousarray(np.broadcast_to(home, (P, ch.dof)))
    return ch, goals, seed, K, (None if limit is None else np.full(ch.dof, limit))


def oracle_search_paths(O, chain, goals, seed, max_attempts, max_joint_step=None, kw=None, **search_kw):
    """the loop over the CPU oracle, in the math mode that is set"""
    o = O.Oracle(chain)
    p = O.default_params(mode=1, **(kw or {}))
    return reference_search_paths(
        lambda g, sd, ig: o.solve_batch(p, g, sd, num_threads=O.max_threads(), initial_guess=ig), chain, goals, seed,
        max_attempts, max_joint_step, **search_kw)


def host_loop(solver, params, goals, seed, max_attempts, max_joint_step=None, start_table=None):
    """What a caller writes today: per attempt one local-mode solve_batch for waypoint 0 and one solve_paths for the
    rest, the closed paths taken out of the batch by hand.  start_table: SR.starts() of the call (the restart states,
    drawn ahead: the loop is charged no time for them).  Returns reached [P]."""
    P, W = goals.shape[:2]
    idx = np.arange(P)
    best = np.full(P, -1, dtype=np.int32)
    for a in range(max_attempts):
        sol, st, _, _ = solver.solve_batch(params, goals[idx, 0], seed[idx], initial_guess=start_table[idx, a])
        ok = st > 0
        reached = ok.astype(np.int32)
        if W > 1 and ok.any():
            reached[ok] += solver.solve_paths(params, goals[idx[ok], 1:], sol[ok], max_joint_step)[4]
        best[idx] = np.maximum(best[idx], reached)
        idx = idx[reached < W]
        if len(idx) == 0:
            break
    return best


def time_call_against_loop(solver, params, goals, seed, max_attempts, max_joint_step, rng_seed, start_table, reps=21):
    """Wall-clock seconds of search_paths and of host_loop on the same paths: both warmed, then alternated `reps`
    times, a host clock around calls that end synchronised.  Returns (median call, median loop, all call, all loop)."""
    import time
    for _ in range(2):
        r = solver.search_paths(params, goals, seed, max_attempts, max_joint_step, rng_seed=rng_seed)[4]
        np.testing.assert_array_equal(r, host_loop(solver, params, goals, seed, max_attempts, max_joint_step, start_table))
    tc, tl = [], []
    for _ in range(reps):
        t0 = time.perf_counter()
        solver.search_paths(params, goals, seed, max_attempts, max_joint_step, rng_seed=rng_seed)
        t1 = time.perf_counter()
        host_loop(solver, params, goals, seed, max_attempts, max_joint_step, start_table)
        t2 = time.perf_counter()
        tc.append(t1 - t0)
        tl.append(t2 - t1)
    return float(np.median(tc)), float(np.median(tl)), tc, tl
