"""Cartesian paths from a pose with a memetic start: the NORMATIVE loop of include/pick_ik_amd.h
(pikamd_search_global_paths) over any pair of callables -- a one-problem global-mode solve (the CPU oracle, or a
handle's own solve_batches with one-record batches: tests/search_global_reference.py) and a local-mode solve_batch for
the waypoint loop of tests/path_reference.py --, the fixtures of the tests, and the loop a caller writes today.  The
restart states are tests/search_reference.py's, the attempt seeds tests/search_global_reference.py's, the classes and
the trace tests/startpath_reference.py's."""
import numpy as np

from tests import path_reference as PR
from tests import search_global_reference as SGR
from tests import search_reference as SR
from tests import startpath_reference as SP

STATS_DTYPE = SR.STATS_DTYPE
NAMES = SP.NAMES
CLASSES = SP.CLASSES
Trace = SP.Trace
counts = SP.counts
RNG_SEED = 1
#: paths of a fixture moved out of reach (the LAST ones, +5 m along x at every waypoint)
FAR = 4
#: case -> (memetic_max_generations, max_attempts, the classes of CLASSES the case reaches under both oracle math
#: modes).  With 12 generations the two-tip case completes no path at a later attempt under "portable": 30, and six
#: attempts; it has no step limit, so no jump.
CASES = {"panda": (12, 4, SP.EVERY_CLASS), "ur5": (12, 4, SP.EVERY_CLASS), "panda_unbounded": (12, 4, SP.EVERY_CLASS),
         "torso_dual_arm": (30, 6, (0, 1, 2, 3, 4))}


def params_kw(case, **more):
    """the budget of the global-mode search tests with the case's generations"""
    kw = dict(SGR.BUDGET, memetic_max_generations=CASES[case][0])
    kw.update(more)
    return kw


def fixture(case, fk_of):
    """(chain, goals [P][W]..., seed [P][dof], max_attempts, max_joint_step [dof] or None): startpath_reference's
    fixture (its goals, home seed and step limit) with the last FAR paths out of reach and the case's attempts"""
    ch, goals, seed, _, step = SP.fixture(case, fk_of)
    goals = np.array(goals, dtype=np.float64)
    goals[len(goals) - FAR:, ..., 0] += 5.0
    return ch, goals, seed, CASES[case][1], step


def reference_search_global_paths(solve_one, solve_local, chain, goals, seed, max_attempts, max_joint_step=None,
                                  rng_seed=0, problem_offset=0, initial_guess=None, trace=False):
    """solve_one(goal [1]..., seed [1][dof], initial_guess [1][dof], rng_seed_a, problem) -> (solution [1][dof],
    status [1], cost [1], stats [1]): ONE global-mode problem with problem_offset = problem;
    solve_local(goal [n]..., seed [n][dof]) -> the same four of a LOCAL-mode solve_batch that starts at its seed.
    goals [P][W][7] or [P][W][n_tips][7], seed [P][dof].  Returns (solution [P][W][dof], status [P][W], cost [P][W],
    stats [P][W], reached [P], attempts [P], totals [P]) and, with trace, a Trace behind them."""
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
        rows_sol = np.repeat(seed[idx][:, None, :], W, axis=1)       # rows 1.. of a failed waypoint 0: the seed,
        rows_st = np.full((n, W), PR.NOT_ATTEMPTED, dtype=np.int32)   # not attempted, cost 0, no statistics
        rows_cost = np.zeros((n, W))
        rows_stats = np.zeros((n, W), dtype=STATS_DTYPE)
        for m, p in enumerate(idx):                                   # (what the call returned: no joint-step test)
            sol0, st0, c0, stats0 = solve_one(goals[p:p + 1, 0], seed[p:p + 1], table[p:p + 1, a],
                                              SGR.attempt_seed(rng_seed, a), problem_offset + int(p))
            rows_sol[m, 0], rows_st[m, 0], rows_cost[m, 0], rows_stats[m, 0] = sol0[0], st0[0], c0[0], stats0[0]
        ok = rows_st[:, 0] > 0
        reached_a = np.where(ok, 1, 0).astype(np.int32)
        if W > 1 and ok.any():
            psol, pst, pcost, pstats, preached = PR.reference_paths(solve_local, goals[idx[ok], 1:], rows_sol[ok, 0],
                                                                    max_joint_step)
            rows_sol[ok, 1:], rows_st[ok, 1:], rows_cost[ok, 1:], rows_stats[ok, 1:] = psol, pst, pcost, pstats
            reached_a[ok] += preached
        tr.attempt_stats.append((idx, rows_stats))
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


def oracle_callables(O, chain, kw):
    """(solve_one, solve_local) over the CPU oracle, in the math mode that is set when they are called"""
    o = O.Oracle(chain)
    p_local = O.default_params(mode=1, **kw)
    return (SGR.oracle_solve_one(O, chain, O.default_params(mode=0, **kw)),
            lambda g, sd: o.solve_batch(p_local, g, sd, num_threads=O.max_threads(), initial_guess=sd))


def oracle_search_global_paths(O, chain, goals, seed, max_attempts, max_joint_step=None, kw=None, **search_kw):
    """the loop over the CPU oracle, in the math mode that is set"""
    one, local = oracle_callables(O, chain, kw or {})
    return reference_search_global_paths(one, local, chain, goals, seed, max_attempts, max_joint_step, **search_kw)


def handle_callables(s, params, params_local):
    """(solve_one, solve_local) over the handle's own solve_batches and solve_batch"""
    return SGR.handle_solve_one(s, params), lambda g, sd: s.solve_batch(params_local, g, sd, initial_guess=sd)


def host_loop(s, params, params_local, goals, seed, max_attempts, max_joint_step, rng_seed, start_table):
    """What a caller writes today: per attempt the open paths compacted by hand, one global-mode solve_batches call
    with one record per open path (its problem_offset is the path's index), a read-back, one solve_paths call on the
    successes, a read-back, a comparison of `reached`.  start_table: SR.starts() of the call (the restart states,
    drawn ahead: the loop is charged no time for them, and a caller could not draw an unbounded variable's at all).
    Returns reached [P]."""
    from pick_ik_amd import solver as S
    P, W = goals.shape[:2]
    idx = np.arange(P)
    best = np.full(P, -1, dtype=np.int32)
    for a in range(max_attempts):
        seed_a = SGR.attempt_seed(rng_seed, a)
        res = []
        for lo in range(0, len(idx), S.MAX_BATCHES):
            part = idx[lo:lo + S.MAX_BATCHES]
            res += s.solve_batches(params, [(goals[p:p + 1, 0], seed[p:p + 1], start_table[p:p + 1, a], int(p))
                                            for p in part], rng_seed=seed_a)
        ok = np.array([r[1][0] > 0 for r in res])
        reached = ok.astype(np.int32)
        if W > 1 and ok.any():
            sol0 = np.stack([r[0][0] for r, good in zip(res, ok) if good])
            reached[ok] += s.solve_paths(params_local, goals[idx[ok], 1:], sol0, max_joint_step)[4]
        best[idx] = np.maximum(best[idx], reached)
        idx = idx[reached < W]
        if len(idx) == 0:
            break
    return best


def time_call_against_loop(s, params, params_local, goals, seed, max_attempts, max_joint_step, rng_seed, start_table,
                           reps=21):
    """startpath_reference.time_call_against_loop's harness for search_global_paths and host_loop: both warmed, then
    alternated `reps` times, a host clock around calls that end synchronised.  Returns (median call, median loop, all
    call, all loop)."""
    import time
    for _ in range(2):
        r = s.search_global_paths(params, goals, seed, max_attempts, max_joint_step, rng_seed=rng_seed)[4]
        np.testing.assert_array_equal(r, host_loop(s, params, params_local, goals, seed, max_attempts, max_joint_step,
                                                   rng_seed, start_table))
    tc, tl = [], []
    for _ in range(reps):
        t0 = time.perf_counter()
        s.search_global_paths(params, goals, seed, max_attempts, max_joint_step, rng_seed=rng_seed)
        t1 = time.perf_counter()
        host_loop(s, params, params_local, goals, seed, max_attempts, max_joint_step, rng_seed, start_table)
        t2 = time.perf_counter()
        tc.append(t1 - t0)
        tl.append(t2 - t1)
    return float(np.median(tc)), float(np.median(tl)), tc, tl
