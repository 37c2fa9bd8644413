"""Memetic IK with random restarts: the NORMATIVE loop of include/pick_ik_amd.h (pikamd_search_global_batch) over any
one-problem solve callable -- the CPU oracle, or a handle's own solve_batches with one-record batches -- and the
fixtures of the global-mode search tests.  The restart draw, the start table and the base fixtures are
tests/search_reference.py's."""
import numpy as np

from tests import search_reference as SR

STATS_DTYPE = SR.STATS_DTYPE
NAMES = SR.NAMES
RNG_SEED = 1
K = 4
MASK64 = (1 << 64) - 1

#: case -> memetic_max_generations: with population 16, elite 4 and 10 descent steps every case has problems solved at
#: the first attempt, at a later one and never (the last 8 targets are out of reach), under both oracle math modes
GENERATIONS = {"panda": 12, "ur5": 12, "panda_unbounded": 12, "panda_on_torso": 12, "torso_dual_arm": 12,
               "floating_panda_fixed_base": 4, "rr": 4}
BUDGET = dict(memetic_population_size=16, memetic_elite_size=4, memetic_gd_max_iters=10)


def attempt_seed(rng_seed, a):
    """rng_seed_a of the header: a added to the HIGH word, mod 2^64"""
    return (int(rng_seed) + (int(a) << 32)) & MASK64


def params_kw(case, **more):
    kw = dict(BUDGET, memetic_max_generations=GENERATIONS[case])
    kw.update(SR.CASES[case][3])
    kw.update(more)
    return kw


def fixture(case, fk_of, B=64, far=8):
    """search_reference.fixture with the last `far` targets moved 5 m along x: out of reach"""
    ch, goals, seed, _ = SR.fixture(case, fk_of, B)
    goals = np.array(goals, dtype=np.float64)
    g = goals.reshape(B, -1, 7)
    if far:
        g[B - far:, :, 0] += 5.0
    return ch, goals, seed


def reference_search(solve_one, chain, goals, seed, max_attempts, rng_seed=0, problem_offset=0, initial_guess=None,
                     all_attempts=False):
    """solve_one(goal [1]..., seed [1][dof], initial_guess [1][dof], rng_seed_a, problem) -> (solution [1][dof],
    status [1], cost [1], stats [1]): ONE global-mode problem with problem_offset = problem.  Returns (solution, status,
    cost, stats, attempts) and, with all_attempts, (all_solution [B][K][dof], all_status [B][K])."""
    goals = np.asarray(goals, dtype=np.float64)
    seed = np.asarray(seed, dtype=np.float64)
    B, dof, Kk = len(seed), chain.dof, max_attempts
    table = SR.starts(chain, seed, Kk, rng_seed, problem_offset, initial_guess)
    solution = np.empty((B, dof))
    status = np.empty(B, dtype=np.int32)
    cost = np.empty(B)
    stats = np.zeros(B, dtype=STATS_DTYPE)
    attempts = np.zeros(B, dtype=np.int32)
    all_solution = np.empty((B, Kk, dof))
    all_status = np.empty((B, Kk), dtype=np.int32)
    for b in range(B):
        is_open = True
        for a in range(Kk):
            if not (is_open or all_attempts):
                break
            sol, st, c, stt = solve_one(goals[b:b + 1], seed[b:b + 1], table[b:b + 1, a], attempt_seed(rng_seed, a),
                                        problem_offset + b)
            all_solution[b, a] = sol[0]
            all_status[b, a] = st[0]
            if not is_open:
                continue
            solution[b] = sol[0]
            status[b] = st[0]
            cost[b] = c[0]
            for f in STATS_DTYPE.names:
                stats[f][b] += stt[f][0]
            attempts[b] = a + 1
            if st[0] > 0:
                is_open = False
    if all_attempts:
        return solution, status, cost, stats, attempts, all_solution, all_status
    return solution, status, cost, stats, attempts


def oracle_solve_one(O, chain, params):
    o = O.Oracle(chain)
    return lambda g, sd, ig, rs, prob: o.solve_batch(params, g, sd, rng_seed=rs, problem_offset=prob, initial_guess=ig)


def oracle_search(O, chain, goals, seed, max_attempts, kw, **search_kw):
    """the loop over the CPU oracle, in the math mode that is set"""
    return reference_search(oracle_solve_one(O, chain, O.default_params(mode=0, **kw)), chain, goals, seed, max_attempts,
                            **search_kw)


def handle_solve_one(s, params):
    """one-record batches through the handle's own solve_batches"""
    def solve(g, sd, ig, rs, prob):
        (r,) = s.solve_batches(params, [(g, sd, ig, prob)], rng_seed=rs)
        return r
    return solve


def host_loop(s, params, goals, seed, max_attempts, rng_seed, start_table):
    """What a caller writes today: up to max_attempts global-mode solve_batches round trips, the failures compacted by
    hand, attempt a with rng_seed_a; one record per call with the call's problems (problem_offset 0: the streams of a
    compacted problem are not the one-record ones -- this is the baseline of the timing test, not a reference).
    Returns (status [B], attempts [B])."""
    B = len(seed)
    idx = np.arange(B)
    status = np.empty(B, dtype=np.int32)
    attempts = np.zeros(B, dtype=np.int32)
    for a in range(max_attempts):
        (r,) = s.solve_batches(params, [(goals[idx], seed[idx], start_table[idx, a], 0)],
                               rng_seed=attempt_seed(rng_seed, a))
        st = r[1]
        status[idx] = st
        attempts[idx] = a + 1
        idx = idx[st <= 0]
        if len(idx) == 0:
            break
    return status, attempts
