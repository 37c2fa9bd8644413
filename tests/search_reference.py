"""Local IK with random restarts: the NORMATIVE loop of include/pick_ik_amd.h (pikamd_search_batch) over any
solve_batch-shaped callable -- the CPU oracle, or a handle's own solve_batch --, the restart draw in numpy, and the
fixture generator of the search tests."""
import dataclasses
import math

import numpy as np

from pick_ik_amd import robots

STREAM_RESTART = 3
#: rng_seed of the fixture tests: with it every case of CASES has problems solved at the first attempt, at a later one
#: and never, under both oracle math modes (tests/test_search_cpu.py asserts it)
RNG_SEED = 1
MAX_ATTEMPTS = 64
STATS_DTYPE = np.dtype([("cost_evals", "<i8"), ("generations", "<i4"), ("wipeouts", "<i4"), ("pool_erasures", "<i4"),
                        ("reserved", "<i4")])
NAMES = ("solution", "status", "cost", "stats", "attempts")


def _u01():
    from oracle import oracle as O
    return O.rng_u01


def draw(chain, rng_seed, problem, epoch, prev):
    """draw(b, e, prev) of the header for global problem index `problem`: every product, sum and difference rounded on
    its own (numpy float64 scalars do)."""
    u01 = _u01()
    out = np.empty(chain.dof)
    pi = np.float64(math.pi)
    for j in range(chain.dof):
        u = np.float64(u01(rng_seed, STREAM_RESTART, problem, epoch, 0, j))
        if chain.bounded[j]:
            lo, hi = np.float64(chain.qmin[j]), np.float64(chain.qmax[j])
        else:
            lo, hi = np.float64(prev[j]) - pi, np.float64(prev[j]) + pi
        out[j] = (hi - lo) * u + lo
    return out


def valid(chain, q):
    """src/pick_ik_plugin.cpp:152-159: every bounded variable within its limits (a NaN is not)"""
    b = np.asarray(chain.bounded, dtype=bool)
    q = np.asarray(q)
    with np.errstate(invalid="ignore"):
        return bool(np.all((q[b] <= np.asarray(chain.qmax)[b]) & (q[b] >= np.asarray(chain.qmin)[b])))


def starts(chain, seed, max_attempts, rng_seed=0, problem_offset=0, initial_guess=None):
    """[B][max_attempts][dof]: where attempt a of problem b starts when every attempt before it failed"""
    seed = np.asarray(seed, dtype=np.float64)
    init = np.array(seed if initial_guess is None else initial_guess, dtype=np.float64)
    B = len(seed)
    out = np.empty((B, max_attempts, chain.dof))
    for b in range(B):
        cur = init[b]
        if not valid(chain, cur):
            cur = draw(chain, rng_seed, problem_offset + b, 0, cur)
        for a in range(max_attempts):
            out[b, a] = cur
            cur = draw(chain, rng_seed, problem_offset + b, a + 1, cur)
    return out


def reference_search(solve, chain, goals, seed, max_attempts, rng_seed=0, problem_offset=0, initial_guess=None,
                     all_attempts=False):
    """solve(goal [n]..., seed [n][dof], initial_guess [n][dof]) -> (solution, status, cost, stats): a LOCAL-mode
    solve_batch.  Returns (solution [B][dof], status [B], cost [B], stats [B], attempts [B]); with all_attempts also
    (all_solution [B][K][dof], all_status [B][K]): one solve from every start, whoever won."""
    goals = np.asarray(goals, dtype=np.float64)
    seed = np.asarray(seed, dtype=np.float64)
    B, dof, K = len(seed), chain.dof, max_attempts
    st0 = starts(chain, seed, K, rng_seed, problem_offset, initial_guess)
    solution = np.empty((B, dof))
    status = np.empty(B, dtype=np.int32)
    cost = np.empty(B)
    stats = np.zeros(B, dtype=STATS_DTYPE)
    attempts = np.zeros(B, dtype=np.int32)
    all_solution = np.empty((B, K, dof))
    all_status = np.empty((B, K), dtype=np.int32)
    is_open = np.ones(B, dtype=bool)
    for a in range(K):
        idx = np.arange(B) if all_attempts else np.nonzero(is_open)[0]
        if len(idx) == 0:
            break
        sol, st, c, stt = solve(goals[idx], seed[idx], st0[idx, a])
        all_solution[idx, a] = sol
        all_status[idx, a] = st
        for n, b in enumerate(idx):
            if not is_open[b]:
                continue
            solution[b] = sol[n]
            status[b] = st[n]
            cost[b] = c[n]
            for f in STATS_DTYPE.names:
                stats[f][b] += stt[f][n]
            attempts[b] = a + 1
            if st[n] > 0:
                is_open[b] = False
    if all_attempts:
        return solution, status, cost, stats, attempts, all_solution, all_status
    return solution, status, cost, stats, attempts


def search_counts(status, attempts):
    """(solved at the first attempt, solved at a later one, never solved)"""
    status, attempts = np.asarray(status), np.asarray(attempts)
    ok = status > 0
    return int((ok & (attempts == 1)).sum()), int((ok & (attempts > 1)).sum()), int((~ok).sum())


def panda_unbounded():
    """the Panda with its first and last variable unbounded (continuous joints): their draws are centred on the
    previous attempt's start"""
    return dataclasses.replace(robots.panda(), bounded=np.array([0, 1, 1, 1, 1, 1, 0], dtype=np.uint8))


def _mid(chain):
    return 0.5 * (np.asarray(chain.qmin) + np.asarray(chain.qmax))


#: name -> (chain, home pose or None = the middle of the limits, variables pinned at their home value, parameters)
CASES = {
    "panda": (robots.panda, robots.PANDA_HOME, (), {}),
    "panda_displacement": (robots.panda, robots.PANDA_HOME, (), dict(minimal_displacement_weight=0.001)),
    "ur5": (robots.ur5, None, (), {}),
    "panda_on_torso": (robots.panda_on_torso, robots.PANDA_ON_TORSO_HOME, (), {}),
    "torso_dual_arm": (robots.torso_dual_arm, None, (), {}),
    "floating_panda_fixed_base": (robots.floating_panda, robots.FLOATING_PANDA_HOME, tuple(range(7)), {}),
    "rr": (robots.rr, None, (), {}),
    "panda_unbounded": (panda_unbounded, robots.PANDA_HOME, (), {}),
}


def fixture(case, fk_of, B=64):
    """(chain, goals [B]..., seed [B][dof], parameters) of one case.  Targets are fk(mid + 0.9 half U(-1, 1)) from
    default_rng(11); an unbounded variable, and one the case pins, takes its home value instead.  Every search starts
    at the home pose.  fk_of(chain) -> fk(q [n][dof])."""
    make, home, pinned, kw = CASES[case]
    ch = make()
    mid = _mid(ch)
    half = 0.5 * (np.asarray(ch.qmax) - np.asarray(ch.qmin))
    home = mid if home is None else np.asarray(home, dtype=np.float64)
    rng = np.random.default_rng(11)
    q = mid + 0.9 * half * rng.uniform(-1.0, 1.0, size=(B, ch.dof))
    fixed = [j for j in range(ch.dof) if not ch.bounded[j] or j in pinned]
    q[:, fixed] = home[fixed]
    goals = np.ascontiguousarray(fk_of(ch)(q))
    seed = np.ascontiguousarray(np.broadcast_to(home, (B, ch.dof)))
    return ch, goals, seed, kw


def oracle_search(O, chain, goals, seed, max_attempts, kw=None, **search_kw):
    """the loop over the CPU oracle, in the math mode that is set"""
    o = O.Oracle(chain)
    p = O.default_params(mode=1, **(kw or {}))
    return reference_search(lambda g, sd, ig: o.solve_batch(p, g, sd, num_threads=O.max_threads(), initial_guess=ig),
                            chain, goals, seed, max_attempts, **search_kw)


def host_loop(solver, params, goals, seed, max_attempts, rng_seed=0, start_table=None):
    """What a caller writes today: up to max_attempts local-mode solve_batch round trips, the solved problems taken
    out of the batch by hand.  start_table: starts() of the call (its restart states, drawn ahead: the loop is charged
    no time for them).  Returns (status [B], attempts [B])."""
    B = len(seed)
    idx = np.arange(B)
    status = np.empty(B, dtype=np.int32)
    attempts = np.zeros(B, dtype=np.int32)
    for a in range(max_attempts):
        _, st, _, _ = solver.solve_batch(params, goals[idx], seed[idx], initial_guess=start_table[idx, a])
        status[idx] = st
        attempts[idx] = a + 1
        idx = idx[st <= 0]
        if len(idx) == 0:
            break
    return status, attempts
