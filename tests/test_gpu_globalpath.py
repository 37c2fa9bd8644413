"""Cartesian paths from a pose with a memetic start on the GPU (pikamd_search_global_paths): waypoint 0 of every
attempt by the memetic solver, the waypoints behind it by the local descents, the start restarted until the path holds.

Its result is DEFINED by the loop of global-mode solve_batches and local-mode solve_paths calls in
include/pick_ik_amd.h (tests/globalpath_reference.py holds that loop), so everything here compares at tolerance zero:
against the loop over the CPU oracle for the exact builds, against the loop over the handle's own calls for every
flavour, every variant of the tail kernel against the one-lane variant.  tests/test_globalpath_cpu.py shows that the
fixtures reach every class of the loop."""
import os
import subprocess
import sys

import numpy as np
import pytest

import pick_ik_amd as pk
from pick_ik_amd import robots
from tests import abi_calls as A
from tests import globalpath_reference as GP
from tests import path_reference as PR
from tests import search_global_reference as SGR
from tests import search_reference as SR
from tests.test_gpu_fuzz import random_chain
from tests.test_gpu_path import FLOATING_BASE, mimic_panda

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUTPUTS = A.STARTPATH_OUTPUTS


@pytest.fixture(scope="module")
def O(oracle_mod):
    import __graft_entry__ as g
    g.build()
    return oracle_mod


def same(a, b, what=""):
    for x, y, w in zip(a, b, GP.NAMES):
        np.testing.assert_array_equal(x, y, err_msg=f"{what}: {w}")


def both(**kw):
    """the parameters of a call and p_local of the header"""
    return pk.default_params(mode=0, **kw), pk.default_params(mode=1, **kw)


def own_loop(s, ch, p, pl, goals, seed, K, step=None, **kw):
    """the normative loop over the handle's own solve_batches and solve_batch"""
    one, local = GP.handle_callables(s, p, pl)
    return GP.reference_search_global_paths(one, local, ch, goals, seed, K, step, **kw)


def raw_call(*args, **kw):
    """pikamd_search_global_paths[_device] as the C ABI takes it (tests/abi_calls.py)"""
    return A.search_paths(*args, global_mode=True, **kw)


fresh_arrays = A.startpath_arrays


_oracle_runs = {}


def oracle_run(O, case, flavour):
    """the loop over the oracle on a fixture, once per (case, math mode); nobody changes what it returns.  Called
    under the exact_flavour fixture: "portable" there means the flavour's own mode."""
    if (case, flavour) not in _oracle_runs:
        with O.math_mode("portable"):
            ch, goals, seed, K, step = GP.fixture(case, lambda c: O.Oracle(c).fk)
            want = GP.oracle_search_global_paths(O, ch, goals, seed, K, step, kw=GP.params_kw(case),
                                                 rng_seed=GP.RNG_SEED, trace=True)
        _oracle_runs[(case, flavour)] = (ch, goals, seed, K, step, want)
    return _oracle_runs[(case, flavour)]


@pytest.mark.parametrize("case", list(GP.CASES))
def test_search_equals_the_loop_over_the_oracle(O, exact_flavour, case):
    """"portable": the verification library against the oracle's plain IEEE mode; "fma": the product library's exact
    kernels (what a default handle of these chains runs with arithmetic = exact) against the oracle's fused mode"""
    ch, goals, seed, K, step, want = oracle_run(O, case, exact_flavour)
    c = GP.counts(want[:7], want[7])
    assert all(c[k] >= 1 for k in GP.CASES[case][2]), (case, exact_flavour, c)
    s = pk.Solver(ch, device=0, strict=True)
    try:
        p = pk.default_params(mode=0, **GP.params_kw(case))
        got = s.search_global_paths(p, goals, seed, K, step, rng_seed=GP.RNG_SEED)
        print(f"{case} [{exact_flavour}] {s.kernel_name(p)} + {s.search_global_paths_kernel_name(p, len(seed))}: " +
              ", ".join(f"{n} {k}" for n, k in zip(c, GP.CLASSES)))
        same(got, want[:7], f"{case} [{exact_flavour}]")
    finally:
        s.close()


@pytest.mark.parametrize("exact", [None, False], ids=["default_exact", "fast"])
@pytest.mark.parametrize("case", list(GP.CASES))
def test_search_equals_the_loop_over_the_handles_own_calls(O, case, exact):
    ch = GP.SP.CASES[case][0]()
    s = pk.Solver(ch, device=0, exact=exact)
    try:
        _, goals, seed, K, step = GP.fixture(case, lambda c: s.fk)
        # (the two-tip case runs 30 generations and six attempts: once)
        for more in ({}, dict(minimal_displacement_weight=0.001))[:1 if case == "torso_dual_arm" else 2]:
            p, pl = both(**GP.params_kw(case, **more))
            want = own_loop(s, ch, p, pl, goals, seed, K, step, rng_seed=GP.RNG_SEED, trace=True)
            got = s.search_global_paths(p, goals, seed, K, step, rng_seed=GP.RNG_SEED)
            same(got, want[:7], f"{case} exact={exact} {more}")
            c = GP.counts(want[:7], want[7])
            print(f"{case} exact={exact} {more} {s.kernel_name(p)} + {s.search_global_paths_kernel_name(p, len(seed))}: {c}")
            assert c[0] >= 1 and c[2] + c[4] >= 1 and (got[5] > 1).any(), (case, exact, more, c)
    finally:
        s.close()


def test_strict_library_and_its_variants(O):
    ch = robots.panda()
    s = pk.Solver(ch, device=0, strict=True)
    try:
        _, goals, seed, K, step = GP.fixture("panda", lambda c: s.fk)
        p, pl = both(**GP.params_kw("panda"))
        want = own_loop(s, ch, p, pl, goals, seed, K, step, rng_seed=GP.RNG_SEED)
        for l, name in ((1, "pik_strict::ik_globalpath_kernel<7,false>"), (4, "pik_strict::ik_globalpath_team_kernel<7,4>"),
                        (16, "pik_strict::ik_globalpath_team_kernel<7,16>")):
            s.set_option("lanes_per_elite", l)
            assert s.search_global_paths_kernel_name(p, len(seed)) == name
            same(s.search_global_paths(p, goals, seed, K, step, rng_seed=GP.RNG_SEED), want, f"strict lanes {l}")
    finally:
        s.close()


@pytest.mark.parametrize("chain", ["floating", "mimic"])
def test_floating_and_mimic_chains(O, chain):
    """the floating_panda_fixed_base chain and a Panda with a mimic joint, joint-space lines, P = 8, W = 3, K = 3: the
    loop over the handle's own calls (these chains run the exact kernels)"""
    ch = robots.floating_panda() if chain == "floating" else mimic_panda()
    s = pk.Solver(ch, device=0)
    try:
        goals, q0 = PR.joint_lines(ch, s.fk, P=8, W=3, fixed=FLOATING_BASE if chain == "floating" else None)
        home = robots.FLOATING_PANDA_HOME if chain == "floating" else 0.5 * (np.asarray(ch.qmin) + np.asarray(ch.qmax))
        seed = np.ascontiguousarray(np.broadcast_to(np.asarray(home, dtype=np.float64), q0.shape))
        goals = np.array(goals)
        goals[-1, ..., 0] += 5.0  # (one path out of reach)
        p, pl = both(**dict(SGR.BUDGET, memetic_max_generations=SGR.GENERATIONS["floating_panda_fixed_base"]))
        want = own_loop(s, ch, p, pl, goals, seed, 3, rng_seed=GP.RNG_SEED)
        got = s.search_global_paths(p, goals, seed, 3, rng_seed=GP.RNG_SEED)
        print(f"{chain}: {s.search_global_paths_kernel_name(p, 8)}, reached {got[4]}, attempts {got[5]}")
        assert "pik_exact::ik_globalpath" in s.search_global_paths_kernel_name(p, 8)
        same(got, want, chain)
        assert got[4][-1] == 0 and got[5][-1] == 3
    finally:
        s.close()


@pytest.mark.parametrize("exact,robot,lanes", [
    (None, "panda", {1: "pik_exact::ik_globalpath_kernel<7,false>", 4: "pik_exact::ik_globalpath_team_kernel<7,4>",
                     16: "pik_exact::ik_globalpath_team_kernel<7,16>"}),
    (False, "panda", {1: "pik::ik_globalpath_kernel<7,false>", 8: "pik::ik_globalpath_wide_kernel<7,8,false>",
                      16: "pik::ik_globalpath_wide_kernel<7,16,false>"}),
    (False, "torso_dual_arm", {1: "pik::ik_globalpath_kernel<9,true>", 8: "pik::ik_globalpath_wide_kernel<9,8,true>",
                               16: "pik::ik_globalpath_wide_kernel<9,16,true>"}),
    (None, "torso_dual_arm", {1: "pik_exact::ik_globalpath_kernel<9,true>", 16: "pik_exact::ik_globalpath_kernel<9,true>"}),
], ids=["exact_panda", "fast_panda", "fast_two_tips", "exact_two_tips"])
def test_every_variant_returns_the_bits_of_the_one_lane_variant(O, exact, robot, lanes):
    ch = robots.by_name(robot)
    s = pk.Solver(ch, device=0, exact=exact)
    try:
        _, goals, seed, K, step = GP.fixture(robot, lambda c: s.fk)
        p, pl = both(**GP.params_kw(robot, minimal_displacement_weight=0.001))
        P = len(seed)
        assert s.self_test(pl, 32) == 0  # (no width switched off on this chain: a forced width is the width that runs)
        served = robot == "panda" or exact is not False or "ik_path_wide_kernel" in s.path_kernel_name(pl, 1)
        s.set_option("lanes_per_elite", 1)
        ref = s.search_global_paths(p, goals, seed, K, step, rng_seed=GP.RNG_SEED)
        assert (ref[5] > 1).any() and (ref[4] == goals.shape[1]).any() and (ref[4] < goals.shape[1]).any()
        for l, name in lanes.items():
            s.set_option("lanes_per_elite", l)
            assert s.search_global_paths_kernel_name(p, P) == (name if served else lanes[1])
            # (the same variant choice as the path family's for p_local)
            assert s.search_global_paths_kernel_name(p, P) == s.path_kernel_name(pl, P).replace("ik_path", "ik_globalpath")
            same(s.search_global_paths(p, goals, seed, K, step, rng_seed=GP.RNG_SEED), ref, f"{robot} exact={exact} lanes {l}")
        s.set_option("lanes_per_elite", None)
        same(s.search_global_paths(p, goals, seed, K, step, rng_seed=GP.RNG_SEED), ref, f"{robot} exact={exact} adaptive")
        # one path, keyed as path 5 of the call
        same(s.search_global_paths(p, goals[5:6], seed[5:6], K, step, rng_seed=GP.RNG_SEED, problem_offset=5),
             [x[5:6] for x in ref], f"{robot} exact={exact} one path")
        assert "ik_globalpath_kernel<" in s.search_global_paths_kernel_name(p, 1 << 20)
    finally:
        s.close()


@pytest.mark.parametrize("exact", [True, False], ids=["exact", "fast"])
@pytest.mark.parametrize("D", [3, 12])
def test_variants_on_generated_chains_with_teams_across_a_wavefront(O, D, exact):
    """a 3-variable and a 12-variable generated chain; P = 1 (one team), 5 (a partly filled wavefront), 17 (teams of 16
    lanes and of 4 straddle wavefronts) and 65 (one lane per path fills a second wavefront with one lane)"""
    ch = random_chain(np.random.default_rng([0x57A7, D]), D)
    s = pk.Solver(ch, device=0, exact=exact)
    try:
        goals, q0 = PR.joint_lines(ch, s.fk, P=65, W=4)
        rng = np.random.default_rng(D)
        seed = q0 + 0.3 * rng.normal(size=q0.shape) * (np.arange(65) % 3 != 0)[:, None]  # (a third start on their line)
        p, pl = both(**dict(SGR.BUDGET, memetic_max_generations=4))
        step = np.full(D, 0.3)
        assert s.self_test(pl, 32) == 0  # (no width switched off on this chain: a forced width is the width that runs)
        for P in (1, 5, 17, 65):
            s.set_option("lanes_per_elite", 1)
            ref = s.search_global_paths(p, goals[:P], seed[:P], 3, step, rng_seed=7)
            assert "ik_globalpath_kernel<" in s.search_global_paths_kernel_name(p, P)
            for l in ((4, 16) if exact else (8, 16)):
                s.set_option("lanes_per_elite", l)
                name = s.search_global_paths_kernel_name(p, P)
                # (a width the chain is not served would fall to one lane and compare that kernel with itself)
                assert name == (f"pik_exact::ik_globalpath_team_kernel<{D},{l}>" if exact else
                                f"pik::ik_globalpath_wide_kernel<{D},{l},false>"), name
                same(s.search_global_paths(p, goals[:P], seed[:P], 3, step, rng_seed=7), ref,
                     f"D = {D} exact={exact} P = {P} lanes {l}: {name}")
            s.set_option("lanes_per_elite", None)
            same(s.search_global_paths(p, goals[:P], seed[:P], 3, step, rng_seed=7), ref, f"D = {D} exact={exact} P = {P} adaptive")
        want = own_loop(s, ch, p, pl, goals, seed, 3, step, rng_seed=7)
        same(ref, want, f"D = {D} exact={exact}: the loop over the handle's own calls")
        print(f"D = {D} exact={exact}: reached {np.bincount(ref[4], minlength=5)}, attempts {np.bincount(ref[5], minlength=4)}")
    finally:
        s.close()


@pytest.mark.parametrize("exact", [None, False], ids=["default_exact", "fast"])
def test_consequences_of_the_loop(O, exact):
    """one waypoint is search_global_batch without a gate; one attempt is one global solve_batch and one solve_paths;
    two waypoints; halves with offsets equal the whole; invalid and NaN guesses are re-drawn at epoch 0"""
    ch = SR.panda_unbounded()
    s = pk.Solver(ch, device=0, exact=exact)
    try:
        _, goals, seed, K, step = GP.fixture("panda_unbounded", lambda c: s.fk)
        p, pl = both(**GP.params_kw("panda_unbounded"))
        P, W = goals.shape[:2]
        # W = 1: the global-mode restart search (a gate on the handle is not applied here)
        s.set_approximate_gate(cost_threshold=1e-12, joint_threshold=1e-12)
        sol, st, cost, stats, reached, attempts, totals = s.search_global_paths(p, goals[:, :1], seed, K, step, rng_seed=GP.RNG_SEED)
        s.clear_approximate_gate()
        b = s.search_global_batch(p, goals[:, 0], seed, K, rng_seed=GP.RNG_SEED)
        solved = b[1] > 0
        # (solved at once and never solved; whether a later attempt solves one depends on the flavour's arithmetic)
        assert (solved & (b[4] == 1)).any() and (~solved).any() and (b[4] > 1).any()
        np.testing.assert_array_equal(sol[:, 0], b[0])
        np.testing.assert_array_equal(st[:, 0], b[1])
        np.testing.assert_array_equal(attempts, b[4])
        np.testing.assert_array_equal(totals, b[3])
        np.testing.assert_array_equal(reached, solved.astype(np.int32))
        np.testing.assert_array_equal(cost[solved, 0], b[2][solved])
        # (a problem that no attempt solved keeps its FIRST attempt's row, the restart search reports its last one)
        first = s.search_global_batch(p, goals[:, 0], seed, 1, rng_seed=GP.RNG_SEED)
        np.testing.assert_array_equal(cost[~solved, 0], first[2][~solved])
        # max_attempts = 1: one global-mode solve_batch (a batch of one record is keyed per problem) + one solve_paths
        one = s.search_global_paths(p, goals, seed, 1, step, rng_seed=GP.RNG_SEED)
        sol0, st0, c0, stats0 = s.solve_batch(p, goals[:, 0], seed, rng_seed=GP.RNG_SEED)
        ok = st0 > 0
        assert ok.any() and not ok.all() and (one[5] == 1).all()
        rest = s.solve_paths(pl, goals[ok, 1:], sol0[ok], step)
        for k, x in enumerate((sol0, st0, c0, stats0)):
            np.testing.assert_array_equal(one[k][:, 0], x, err_msg=f"one attempt, row 0: {GP.NAMES[k]}")
        for k in range(4):
            np.testing.assert_array_equal(one[k][ok, 1:], rest[k], err_msg=f"one attempt: {GP.NAMES[k]}")
        np.testing.assert_array_equal(one[4][ok], 1 + rest[4])
        assert (one[4][~ok] == 0).all() and (one[1][~ok, 1:] == PR.NOT_ATTEMPTED).all()
        np.testing.assert_array_equal(one[0][~ok], np.repeat(seed[~ok][:, None], W, axis=1))
        # W = 2
        same(s.search_global_paths(p, goals[:, :2], seed, K, step, rng_seed=GP.RNG_SEED),
             own_loop(s, ch, p, pl, goals[:, :2], seed, K, step, rng_seed=GP.RNG_SEED), f"W = 2 exact={exact}")
        # halves with matching offsets
        whole = s.search_global_paths(p, goals, seed, K, step, rng_seed=5)
        lo = s.search_global_paths(p, goals[:20], seed[:20], K, step, rng_seed=5, problem_offset=0)
        hi = s.search_global_paths(p, goals[20:], seed[20:], K, step, rng_seed=5, problem_offset=20)
        other = s.search_global_paths(p, goals[20:], seed[20:], K, step, rng_seed=5, problem_offset=0)
        same(whole, [np.concatenate([a, b]) for a, b in zip(lo, hi)], f"halves exact={exact}")
        assert not np.array_equal(other[0], hi[0])  # (the offset keys the memetic streams and the restarts)
        # an invalid initial guess (a NaN, a variable outside its limits) is re-drawn at epoch 0
        guess = seed.copy()
        guess[::3, 1] = np.nan
        guess[1::3, 3] = ch.qmax[3] + 0.5
        got = s.search_global_paths(p, goals, seed, K, step, rng_seed=5, initial_guess=guess)
        same(got, own_loop(s, ch, p, pl, goals, seed, K, step, rng_seed=5, initial_guess=guess), f"invalid guesses exact={exact}")
        # a step limit with non-positive entries limits nothing there; none at all
        mixed = np.where(np.arange(ch.dof) % 2 == 0, 0.15, -1.0)
        same(s.search_global_paths(p, goals, seed, K, mixed, rng_seed=5),
             own_loop(s, ch, p, pl, goals, seed, K, mixed, rng_seed=5), f"mixed step limit exact={exact}")
        free = s.search_global_paths(p, goals, seed, K, None, rng_seed=5)
        same(free, own_loop(s, ch, p, pl, goals, seed, K, None, rng_seed=5), f"no step limit exact={exact}")
        same(s.search_global_paths(p, goals, seed, K, np.full(ch.dof, -1.0), rng_seed=5), free, "a limit of -1 is none")
        assert not (free[1] == PR.PATH_JUMP).any() and (whole[1] == PR.PATH_JUMP).any()
    finally:
        s.close()


def test_attempt_edges(O):
    """K = 64 with 2 generations; every path out of reach; return_approximate_solution: every path is solved at attempt
    0 without a step limit, and with one only a refused jump reopens a path"""
    ch = robots.panda()
    s = pk.Solver(ch, device=0)
    try:
        _, goals, seed, _, step = GP.fixture("panda", lambda c: s.fk)
        goals, seed = np.ascontiguousarray(goals[:5, :3]), np.ascontiguousarray(seed[:5])
        p, pl = both(**dict(SGR.BUDGET, memetic_max_generations=2))
        got = s.search_global_paths(p, goals, seed, 64, step, rng_seed=GP.RNG_SEED)
        same(got, own_loop(s, ch, p, pl, goals, seed, 64, step, rng_seed=GP.RNG_SEED), "K = 64")
        assert (got[5] > 4).any()
        far = goals.copy()
        far[..., 0] += 5.0
        sol, st, cost, stats, reached, attempts, totals = s.search_global_paths(p, far, seed, 5, step, rng_seed=GP.RNG_SEED)
        same((sol, st, cost, stats, reached, attempts, totals), own_loop(s, ch, p, pl, far, seed, 5, step, rng_seed=GP.RNG_SEED), "out of reach")
        assert (reached == 0).all() and (attempts == 5).all() and (st[:, 0] == pk.NO_IK_SOLUTION).all()
        assert (st[:, 1:] == PR.NOT_ATTEMPTED).all()
        np.testing.assert_array_equal(sol, np.repeat(seed[:, None], 3, axis=1))
        # servo mode on unreachable lines: every waypoint returns its best configuration, which is held
        pa, pla = both(**dict(SGR.BUDGET, memetic_max_generations=2, return_approximate_solution=1))
        s.set_approximate_gate(cost_threshold=1e-12, joint_threshold=1e-12)  # (not applied)
        got = s.search_global_paths(pa, far, seed, 4, None, rng_seed=GP.RNG_SEED)
        s.clear_approximate_gate()
        same(got, own_loop(s, ch, pa, pla, far, seed, 4, None, rng_seed=GP.RNG_SEED), "servo, no limit")
        assert (got[5] == 1).all() and (got[4] == 3).all() and (got[1] == pk.APPROXIMATE).all()
        tight = np.full(ch.dof, 1e-4)
        got = s.search_global_paths(pa, far, seed, 4, tight, rng_seed=GP.RNG_SEED)
        want = own_loop(s, ch, pa, pla, far, seed, 4, tight, rng_seed=GP.RNG_SEED, trace=True)
        same(got, want[:7], "servo, step limit")
        assert (got[4] >= 1).all() and (want[7].jumped | (got[5] == 1)).all() and want[7].jumped.any()
    finally:
        s.close()


def test_device_entry_point_streams_and_slots():
    """search_global_paths_device on a non-default stream equals the host-pointer call; a smaller call behind it on the
    same slot; two slots in flight on two streams equal their serial answers (own interpreter: torch allocates the
    buffers)"""
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "globalpath_device_check.py")], cwd=ROOT,
                       capture_output=True, text=True, timeout=900)
    assert r.returncode == 0 and "globalpath device check OK" in r.stdout, r.stdout[-2000:] + r.stderr[-3000:]


def test_every_optional_array_may_be_absent(O):
    """P = 3 paths of W = 3 waypoints (odd row counts: the int32 arrays end off an 8-byte boundary): the call with
    every optional array, then with each one NULL in turn -- every array still given is the full call's, bit for bit
    (the initial guess given is the seed and the step limit "no limit": leaving them out changes no answer) --, then
    with all of them NULL at once"""
    ch = robots.panda()
    s = pk.Solver(ch, device=0)
    try:
        _, goals, seed, K, _ = GP.fixture("panda", lambda c: s.fk)
        goals, seed = np.ascontiguousarray(goals[5:8, :3]), np.ascontiguousarray(seed[5:8])
        p = pk.default_params(mode=0, **dict(SGR.BUDGET, memetic_max_generations=3))
        optional = ("final_cost", "stats", "reached", "attempts", "totals", "initial_guess", "max_joint_step")
        full = A.check_optional_arrays(
            lambda a: raw_call(s._L, s._h, p, 3, 3, K, a, rng_seed=GP.RNG_SEED),
            lambda: fresh_arrays(s, goals, seed, seed.copy(), np.full(ch.dof, -1.0)), optional, OUTPUTS)
        same([full[k] for k in OUTPUTS], s.search_global_paths(p, goals, seed, K, rng_seed=GP.RNG_SEED), "binding")
        assert (full["attempts"] > 1).any()  # (rows went through the slot's scratch)
        bare = fresh_arrays(s, goals, seed, None, None)
        bare.update({k: None for k in optional})
        assert raw_call(s._L, s._h, p, 3, 3, K, bare, rng_seed=GP.RNG_SEED) == 0
        np.testing.assert_array_equal(bare["solution"], full["solution"])
        np.testing.assert_array_equal(bare["status"], full["status"])
    finally:
        s.close()


def test_refusals(O):
    ch = robots.panda()
    s = pk.Solver(ch, device=0)
    L, h = s._L, s._h
    try:
        _, goals, seed, K, step = GP.fixture("panda", lambda c: s.fk)
        goals, seed = np.ascontiguousarray(goals[:6]), np.ascontiguousarray(seed[:6])
        P, W = goals.shape[:2]
        p = pk.default_params(mode=0, **GP.params_kw("panda"))
        ref = s.search_global_paths(p, goals, seed, K, step, rng_seed=GP.RNG_SEED)
        # no path: nothing to do
        e = s.search_global_paths(p, np.zeros((0, 5, 7)), np.zeros((0, 7)), 3)
        assert e[0].shape == (0, 5, 7) and e[1].shape == (0, 5) and e[4].shape == (0,) and e[6].shape == (0,)
        err = lambda: L.pikamd_last_error().decode()  # noqa: E731

        def raw(params, P_=P, W_=W, K_=K, **gone):
            a = fresh_arrays(s, goals, seed, None, step)
            a.update(gone)
            return raw_call(L, h, params, P_, W_, K_, a)

        assert raw(p) == 0
        # refusals: PIKAMD_EINVAL (-1) and a message
        assert raw(pk.default_params(mode=1)) == -1 and "pikamd_search_paths" in err() and "mode = 0" in err()
        assert raw(p, W_=0) == -1 and "W >= 1" in err()
        assert raw(p, P_=-1) == -1 and "P >= 0" in err()
        for k in (0, 65):
            assert raw(p, K_=k) == -1 and "max_attempts" in err(), k
        for missing in ("goal", "seed", "solution", "status"):
            assert raw(p, **{missing: None}) == -1 and "must not be NULL" in err(), missing
        assert raw(p, P_=0, goal=None, seed=None, solution=None, status=None) == 0
        assert raw_call(L, h, p, 4, 1, 1, {}, device=True) == -1
        assert raw_call(L, h, p, 0, 1, 1, {}, device=True, slot=999) == -1 and "slot" in err()
        assert raw_call(L, None, p, 4, 1, 1, {}) == -1 and raw_call(L, h, None, 4, 1, 1, {}) == -1
        with pytest.raises(pk.PickIkAmdError, match="pikamd_search_paths"):
            s.search_global_paths(pk.default_params(mode=1), goals, seed, K)
        s.set_option("joint_layout", "soa")
        with pytest.raises(pk.PickIkAmdError, match="joint_layout soa"):
            s.search_global_paths(p, goals, seed, K)
        s.set_option("joint_layout", "aos")
        same(s.search_global_paths(p, goals, seed, K, step, rng_seed=GP.RNG_SEED), ref, "after the refusals")
    finally:
        s.close()


def test_cpp_host_mirror_search_global_paths():
    """tests/native/globalpath_check.cpp: Solver::ik_memetic_search_paths against the C ABI call and, with one attempt,
    against the batch and path calls it is defined by"""
    import __graft_entry__ as g
    g.build()
    src = os.path.join(ROOT, "tests", "native", "globalpath_check.cpp")
    exe = os.path.join(ROOT, "tests", "native", "globalpath_check")
    lib_dir = os.path.join(ROOT, "pick_ik_amd")
    if not os.path.exists(exe) or os.path.getmtime(exe) < max(
            os.path.getmtime(src), os.path.getmtime(os.path.join(lib_dir, "host", "pick_ik_amd.hpp"))):
        subprocess.run(["g++", "-std=c++17", "-O1", "-pthread", "-Wall", "-Wextra", "-Werror", src, "-o", exe,
                        "-L" + lib_dir, "-lpick_ik_amd", "-Wl,-rpath," + lib_dir, "-Wl,-rpath,/opt/rocm/lib"], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "globalpath C++ checks OK" in r.stdout, r.stdout + r.stderr


def test_one_call_beats_the_loop_of_round_trips(O):
    """The Panda fixture (48 straight lines of 6 waypoints from the home pose, the last 4 out of reach, up to 4
    attempts of 12 generations, step limit 0.15; the default exact handle): one call against the loop a caller writes
    today -- per attempt the open paths compacted, one global-mode solve_batches call with a record per open path, one
    solve_paths on the successes, the restart states drawn ahead -- in the same process, both warmed, alternated 21
    times, medians of a host clock around calls that end synchronised.  Both sides return the same `reached`, so they
    do the same work.  The baseline is existing, unchanged code and no margin is added.  (Figures of a run:
    profiles/globalpath_latency.txt.)"""
    ch = robots.panda()
    s = pk.Solver(ch, device=0)
    try:
        _, goals, seed, K, step = GP.fixture("panda", lambda c: s.fk)
        p, pl = both(**GP.params_kw("panda"))
        table = SR.starts(ch, seed, K, GP.RNG_SEED)
        call, loop, _, _ = GP.time_call_against_loop(s, p, pl, goals, seed, K, step, GP.RNG_SEED, table, reps=21)
        print(f"P = 48, W = 6, K = {K} [{s.kernel_name(p)} + {s.search_global_paths_kernel_name(p, len(seed))}]: "
              f"search_global_paths {call * 1e3:.3f} ms, loop of solve_batches + solve_paths {loop * 1e3:.3f} ms, "
              f"ratio {loop / call:.2f}")
        assert call < loop, (call, loop)
    finally:
        s.close()
