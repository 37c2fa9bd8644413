"""The approximate-solution gate (src/pick_ik_plugin.cpp:219-267): the NORMATIVE code of include/pick_ik_amd.h
(pikamd_gate_batch, pikamd_set_approximate_gate) -- the gate over any cost-shaped callable (the CPU oracle's cost, or a
handle's own), and the gated loops of both search families, built on tests/search_reference.py and
tests/search_global_reference.py by gating what their solve callables return."""
import dataclasses

import numpy as np

from tests import search_global_reference as GR
from tests import search_reference as SR

GATE_REFUSED = -1002
JOINT_GOAL_WEIGHTS = ("center_joints_weight", "avoid_joint_limits_weight", "minimal_displacement_weight")
#: the fixture of the gate tests: the `panda` case of search_reference with these parameters, rng_seed 1, 8 attempts
K = 8
PANDA_KW = dict(minimal_displacement_weight=0.001, cost_threshold=3e-4, return_approximate_solution=1)
#: ... and the small global-mode budget (population 16, 6 generations, 10 descent iterations), 4 attempts
K_GLOBAL = 4
GLOBAL_KW = dict(memetic_population_size=16, memetic_elite_size=4, memetic_max_generations=6, memetic_gd_max_iters=10)


@dataclasses.dataclass
class Gate:
    cost_threshold: float = 0.0   # approximate_solution_cost_threshold; <= 0: no goal is tested
    joint_threshold: float = 0.0  # approximate_solution_joint_threshold; not > 0: no limit


PANDA_GATE = Gate(6e-4, 2.5)


def gate_params(params, gate):
    """p' of the header: a copy of `params` with the gate's cost threshold when that is > 0, else without joint goals"""
    p = type(params).from_buffer_copy(params)
    if gate.cost_threshold > 0:
        p.cost_threshold = gate.cost_threshold
    else:
        for w in JOINT_GOAL_WEIGHTS:
            setattr(p, w, 0.0)
    return p


def solution_test(cost, params, gate, goals, seed, q):
    """is_solution of cost(p', goal [n]..., seed [n][dof], q [n][dof]) -> (cost [n], is_solution [n])"""
    return np.asarray(cost(gate_params(params, gate), goals, seed, q)[1]) != 0


def joint_test(gate, seed, q):
    """no variable further than the joint threshold from the seed; written as the reference writes it: a NaN threshold
    limits nothing, a NaN difference does not trip the limit"""
    q, seed = np.asarray(q, dtype=np.float64), np.asarray(seed, dtype=np.float64)
    if not gate.joint_threshold > 0:
        return np.ones(len(q), dtype=bool)
    with np.errstate(invalid="ignore"):
        return ~(np.abs(q - seed) > gate.joint_threshold).any(axis=1)


def gate_pass(cost, params, gate, goals, seed, q):
    """pass [n] of pikamd_gate_batch"""
    return solution_test(cost, params, gate, goals, seed, q) & joint_test(gate, seed, q)


def gated(solve, cost, params, gate):
    """The step the gate adds behind a solve: solve(goals, seed, ...) -> (solution, status, cost, stats) with every
    answer of status > 0 that the gate refuses turned into (seed, GATE_REFUSED); cost and stats stay.  No gate, or a call
    without return_approximate_solution: `solve` itself."""
    if gate is None or not params.return_approximate_solution:
        return solve

    def gated_solve(goals, seed, *rest):
        sol, st, c, stats = solve(goals, seed, *rest)
        sol, st = np.array(sol), np.array(st)
        idx = np.nonzero(st > 0)[0]
        if len(idx):
            bad = idx[~gate_pass(cost, params, gate, np.asarray(goals)[idx], np.asarray(seed)[idx], sol[idx])]
            st[bad] = GATE_REFUSED
            sol[bad] = np.asarray(seed)[bad]
        return sol, st, c, stats
    return gated_solve


def gated_search(solve, cost, params, gate, chain, goals, seed, max_attempts, **search_kw):
    """the gated loop of pikamd_search_batch: solve is a LOCAL-mode solve_batch-shaped callable (search_reference)"""
    return SR.reference_search(gated(solve, cost, params, gate), chain, goals, seed, max_attempts, **search_kw)


def gated_search_global(solve_one, cost, params, gate, chain, goals, seed, max_attempts, **search_kw):
    """the gated loop of pikamd_search_global_batch: solve_one as in search_global_reference"""
    return GR.reference_search(gated(solve_one, cost, params, gate), chain, goals, seed, max_attempts, **search_kw)


def oracle_cost(o):
    """the oracle's cost as a batch callable (its own takes ONE goal and seed for n candidates)"""
    def cost(params, goals, seed, q):
        goals, seed, q = np.asarray(goals), np.asarray(seed), np.asarray(q)
        rows = [o.cost(params, goals[i], seed[i], q[i]) for i in range(len(q))]
        return (np.array([r[0][0] for r in rows], dtype=np.float64), np.array([r[1][0] for r in rows], dtype=np.int32))
    return cost


def oracle_search(O, chain, goals, seed, max_attempts, kw, gate, **search_kw):
    """the gated local-mode loop over the CPU oracle, in the math mode that is set"""
    o = O.Oracle(chain)
    p = O.default_params(mode=1, **kw)
    return gated_search(lambda g, sd, ig: o.solve_batch(p, g, sd, num_threads=O.max_threads(), initial_guess=ig),
                        oracle_cost(o), p, gate, chain, goals, seed, max_attempts, **search_kw)


def oracle_search_global(O, chain, goals, seed, max_attempts, kw, gate, **search_kw):
    """... and the global-mode one"""
    o = O.Oracle(chain)
    p = O.default_params(mode=0, **kw)
    return gated_search_global(GR.oracle_solve_one(O, chain, p), oracle_cost(o), p, gate, chain, goals, seed, max_attempts,
                               **search_kw)


def handle_search(s, p, gate, chain, goals, seed, max_attempts, **search_kw):
    """the gated local-mode loop over a handle's own solve_batch and gate: the definition, for every flavour"""
    return SR.reference_search(_handle_gated(lambda g, sd, ig: s.solve_batch(p, g, sd, initial_guess=ig), s, p, gate),
                               chain, goals, seed, max_attempts, **search_kw)


def handle_search_global(s, p, gate, chain, goals, seed, max_attempts, **search_kw):
    return GR.reference_search(_handle_gated(GR.handle_solve_one(s, p), s, p, gate), chain, goals, seed, max_attempts,
                               **search_kw)


def _handle_gated(solve, s, p, gate):
    if gate is None or not p.return_approximate_solution:
        return solve

    def gated_solve(goals, seed, *rest):
        sol, st, c, stats = solve(goals, seed, *rest)
        sol, st = np.array(sol), np.array(st)
        idx = np.nonzero(st > 0)[0]
        if len(idx):
            ok = s.gate(p, handle_gate(gate), np.asarray(goals)[idx], np.asarray(seed)[idx], sol[idx])
            bad = idx[~ok]
            st[bad] = GATE_REFUSED
            sol[bad] = np.asarray(seed)[bad]
        return sol, st, c, stats
    return gated_solve


def handle_gate(gate):
    import pick_ik_amd as pk
    return pk.Gate(gate.cost_threshold, gate.joint_threshold)


def attempt0_classes(cost, params, gate, goals, seed, sol, st):
    """Of the UNGATED answers (sol, st) of attempt 0, boolean masks: accepted with status 1, accepted with status 2,
    refused by the solution test, refused by the joint limit alone (the order the reference tests in)."""
    solved = st > 0
    test = solution_test(cost, params, gate, goals, seed, sol)
    joint = joint_test(gate, seed, sol)
    ok = solved & test & joint
    return ok & (st == 1), ok & (st == 2), solved & ~test, solved & test & ~joint
