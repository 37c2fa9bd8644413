"""Cartesian paths from a pose on the GPU (pikamd_search_paths): the start state restarted until the path holds, in
one launch.

Its result is DEFINED by the loop of local-mode solve_batch and solve_paths calls in include/pick_ik_amd.h
(tests/startpath_reference.py holds that loop), so everything here compares at tolerance zero: against the loop over
the CPU oracle for the exact builds, against the loop over the handle's own calls for the fast flavour, every kernel
variant against every other.  tests/test_startpath_cpu.py shows that the fixtures reach every class of the loop."""
import os
import subprocess
import sys

import numpy as np
import pytest

import pick_ik_amd as pk
from pick_ik_amd import robots
from tests import abi_calls as A
from tests import path_reference as PR
from tests import search_reference as SR
from tests import startpath_reference as SP
from tests.test_gpu_fuzz import random_chain

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUTPUTS = A.STARTPATH_OUTPUTS


@pytest.fixture(scope="module")
def O(oracle_mod):
    import __graft_entry__ as g
    g.build()
    return oracle_mod


def same(a, b, what=""):
    for x, y, w in zip(a, b, SP.NAMES):
        np.testing.assert_array_equal(x, y, err_msg=f"{what}: {w}")


def own_solve(s, p):
    return lambda g, sd, ig: s.solve_batch(p, g, sd, initial_guess=ig)


#: pikamd_search_paths[_device] as the C ABI takes it, and every array of a call (tests/abi_calls.py)
raw_call = A.search_paths
fresh_arrays = A.startpath_arrays


@pytest.mark.parametrize("case", list(SP.CASES))
def test_search_paths_equal_the_loop_over_the_oracle(O, exact_flavour, case):
    """"portable": the verification library against the oracle's plain IEEE mode; "fma": the product library's exact
    kernels (what a default handle of these chains runs with arithmetic = exact) against the oracle's fused mode"""
    with O.math_mode("portable"):
        ch, goals, seed, K, step = SP.fixture(case, lambda c: O.Oracle(c).fk)
        want = SP.oracle_search_paths(O, ch, goals, seed, K, step, rng_seed=SP.RNG_SEED, trace=True)
    c = SP.counts(want[:7], want[7])
    SP.assert_classes(case, c, exact_flavour)
    s = pk.Solver(ch, device=0, strict=True)
    try:
        p = pk.default_params(mode=1)
        got = s.search_paths(p, goals, seed, K, step, rng_seed=SP.RNG_SEED)
        print(f"{case} [{exact_flavour}] {s.search_paths_kernel_name(p, len(seed))}: " +
              ", ".join(f"{n} {k}" for n, k in zip(c, SP.CLASSES)))
        same(got, want[:7], f"{case} [{exact_flavour}]")
    finally:
        s.close()


@pytest.mark.parametrize("exact", [None, False], ids=["default_exact", "fast"])
@pytest.mark.parametrize("case", ["panda", "torso_dual_arm", "panda_unbounded"])
def test_search_paths_equal_the_loop_over_the_handles_own_calls(O, case, exact):
    ch = SP.CASES[case][0]()
    s = pk.Solver(ch, device=0, exact=exact)
    try:
        _, goals, seed, K, step = SP.fixture(case, lambda c: s.fk)
        for kw in ({}, dict(minimal_displacement_weight=0.001)):
            p = pk.default_params(mode=1, **kw)
            want = SP.reference_search_paths(own_solve(s, p), ch, goals, seed, K, step, rng_seed=SP.RNG_SEED, trace=True)
            got = s.search_paths(p, goals, seed, K, step, rng_seed=SP.RNG_SEED)
            same(got, want[:7], f"{case} exact={exact} {kw}")
            c = SP.counts(want[:7], want[7])
            print(f"{case} exact={exact} {kw}: {c}")
            assert c[0] + c[1] >= 1 and c[2] + c[4] >= 1 and (got[5] > 1).any(), (case, exact, kw, c)
    finally:
        s.close()


@pytest.mark.parametrize("exact,robot,lanes", [
    (None, "panda", {1: "pik_exact::ik_startpath_kernel<7,false>", 4: "pik_exact::ik_startpath_team_kernel<7,4>",
                     16: "pik_exact::ik_startpath_team_kernel<7,16>"}),
    (False, "panda", {1: "pik::ik_startpath_kernel<7,false>", 8: "pik::ik_startpath_wide_kernel<7,8,false>",
                      16: "pik::ik_startpath_wide_kernel<7,16,false>"}),
    (False, "torso_dual_arm", {1: "pik::ik_startpath_kernel<9,true>", 8: "pik::ik_startpath_wide_kernel<9,8,true>",
                               16: "pik::ik_startpath_wide_kernel<9,16,true>"}),
    (None, "torso_dual_arm", {1: "pik_exact::ik_startpath_kernel<9,true>", 16: "pik_exact::ik_startpath_kernel<9,true>"}),
], ids=["exact_panda", "fast_panda", "fast_two_tips", "exact_two_tips"])
def test_every_variant_returns_the_same_bits(O, exact, robot, lanes):
    ch = robots.by_name(robot)
    s = pk.Solver(ch, device=0, exact=exact)
    try:
        _, goals, seed, K, _ = SP.fixture(robot, lambda c: s.fk)
        p = pk.default_params(mode=1, minimal_displacement_weight=0.001)
        step = np.full(ch.dof, 0.15)
        P = len(seed)
        ref = s.search_paths(p, goals, seed, K, step, rng_seed=SP.RNG_SEED)  # the adaptive choice
        assert (ref[5] > 1).any() and (ref[4] == goals.shape[1]).any() and (ref[4] < goals.shape[1]).any()
        assert s.self_test(p, 32) == 0  # (no width switched off on this chain: a forced width is the width that runs)
        served = robot == "panda" or exact is not False or "ik_startpath_wide_kernel" in s.search_paths_kernel_name(p, 1)
        for l, name in lanes.items():
            s.set_option("lanes_per_elite", l)
            assert s.search_paths_kernel_name(p, P) == (name if served else lanes[1])
            # (the same variant choice as the path family's)
            assert s.search_paths_kernel_name(p, P) == s.path_kernel_name(p, P).replace("ik_path", "ik_startpath")
            same(s.search_paths(p, goals, seed, K, step, rng_seed=SP.RNG_SEED), ref, f"{robot} exact={exact} lanes {l}")
        s.set_option("lanes_per_elite", None)
        one = s.search_paths_kernel_name(p, 1)
        if robot == "panda":
            assert "ik_startpath_team_kernel" in one or "ik_startpath_wide_kernel" in one, one
        # one path, keyed as path 5 of the call
        same(s.search_paths(p, goals[5:6], seed[5:6], K, step, rng_seed=SP.RNG_SEED, problem_offset=5),
             [x[5:6] for x in ref], f"{robot} exact={exact} one path")
        assert "ik_startpath_kernel<" in s.search_paths_kernel_name(p, 1 << 20)
    finally:
        s.close()


@pytest.mark.parametrize("exact", [True, False], ids=["exact", "fast"])
@pytest.mark.parametrize("D", [3, 12])
def test_variants_on_generated_chains_with_teams_across_a_wavefront(O, D, exact):
    """a 3-variable and a 12-variable generated chain; P = 5 (a partly filled wavefront) and P = 70 (teams of 4, 8 and
    16 lanes straddle the wavefronts, one lane per path fills a second one partly)"""
    ch = random_chain(np.random.default_rng([0x57A7, D]), D)
    s = pk.Solver(ch, device=0, exact=exact)
    try:
        goals, q0 = PR.joint_lines(ch, s.fk, P=70, W=4)
        rng = np.random.default_rng(D)
        seed = q0 + 0.3 * rng.normal(size=q0.shape) * (np.arange(70) % 3 != 0)[:, None]  # (a third start on their line)
        p = pk.default_params(mode=1)
        step = np.full(D, 0.3)
        for P in (5, 70):
            s.set_option("lanes_per_elite", 1)
            ref = s.search_paths(p, goals[:P], seed[:P], 4, step, rng_seed=7)
            assert "ik_startpath_kernel<" in s.search_paths_kernel_name(p, P)
            for l in ((4, 16) if exact else (8, 16)):
                s.set_option("lanes_per_elite", l)
                name = s.search_paths_kernel_name(p, P)
                assert "ik_startpath" in name, name
                same(s.search_paths(p, goals[:P], seed[:P], 4, step, rng_seed=7), ref, f"D = {D} exact={exact} P = {P} lanes {l}: {name}")
            s.set_option("lanes_per_elite", None)
            same(s.search_paths(p, goals[:P], seed[:P], 4, step, rng_seed=7), ref, f"D = {D} exact={exact} P = {P} adaptive")
        want = SP.reference_search_paths(own_solve(s, p), ch, goals, seed, 4, step, rng_seed=7)
        same(ref, want, f"D = {D} exact={exact}: the loop over the handle's own calls")
        print(f"D = {D} exact={exact}: reached {np.bincount(ref[4], minlength=5)}, attempts {np.bincount(ref[5], minlength=5)}")
    finally:
        s.close()


def test_strict_library_variants(O):
    ch = robots.panda()
    s = pk.Solver(ch, device=0, strict=True)
    try:
        _, goals, seed, K, step = SP.fixture("panda", lambda c: s.fk)
        p = pk.default_params(mode=1)
        ref = s.search_paths(p, goals, seed, K, step, rng_seed=SP.RNG_SEED)
        for l, name in ((1, "pik_strict::ik_startpath_kernel<7,false>"), (4, "pik_strict::ik_startpath_team_kernel<7,4>"),
                        (16, "pik_strict::ik_startpath_team_kernel<7,16>")):
            s.set_option("lanes_per_elite", l)
            assert s.search_paths_kernel_name(p, len(seed)) == name
            same(s.search_paths(p, goals, seed, K, step, rng_seed=SP.RNG_SEED), ref, f"strict lanes {l}")
    finally:
        s.close()


@pytest.mark.parametrize("exact", [None, False], ids=["default_exact", "fast"])
def test_consequences_of_the_loop(O, exact):
    """one waypoint is search_batch without a gate; one attempt without a step limit is solve_paths from the seed;
    halves with offsets equal the whole"""
    ch = SR.panda_unbounded()
    s = pk.Solver(ch, device=0, exact=exact)
    try:
        _, goals, seed, K, step = SP.fixture("panda_unbounded", lambda c: s.fk)
        p = pk.default_params(mode=1)
        # W = 1: the restart search (a gate on the handle is not applied here)
        s.set_approximate_gate(cost_threshold=1e-12, joint_threshold=1e-12)
        sol, st, cost, stats, reached, attempts, totals = s.search_paths(p, goals[:, :1], seed, K, step, rng_seed=SP.RNG_SEED)
        s.clear_approximate_gate()
        b = s.search_batch(p, goals[:, 0], seed, K, rng_seed=SP.RNG_SEED)
        first, later, never = SR.search_counts(b[1], b[4])
        assert first >= 1 and later >= 1 and never >= 1, (first, later, never)
        solved = b[1] > 0
        np.testing.assert_array_equal(sol[:, 0], b[0])
        np.testing.assert_array_equal(st[:, 0], b[1])
        np.testing.assert_array_equal(attempts, b[4])
        np.testing.assert_array_equal(totals, b[3])
        np.testing.assert_array_equal(reached, solved.astype(np.int32))
        np.testing.assert_array_equal(cost[solved, 0], b[2][solved])
        # (a problem that no attempt solved keeps its FIRST attempt's row, the restart search reports its last one)
        np.testing.assert_array_equal(cost[~solved, 0], s.solve_batch(p, goals[~solved, 0], seed[~solved])[2])
        # max_attempts = 1, no step limit: the path call from the seed (its first waypoint has a valid guess: the seed)
        one = s.search_paths(p, goals, seed, 1)
        paths = s.solve_paths(p, goals, seed)
        for x, y, w in zip(one[:5], paths, SP.NAMES):
            np.testing.assert_array_equal(x, y, err_msg=f"one attempt: {w}")
        assert (one[5] == 1).all()
        np.testing.assert_array_equal(one[6]["cost_evals"], paths[3]["cost_evals"].sum(axis=1))
        np.testing.assert_array_equal(one[6]["generations"], paths[3]["generations"].sum(axis=1))
        assert 0 < (one[4] == goals.shape[1]).sum() < len(seed)
        # halves with matching offsets
        whole = s.search_paths(p, goals, seed, K, step, rng_seed=5)
        lo = s.search_paths(p, goals[:20], seed[:20], K, step, rng_seed=5, problem_offset=0)
        hi = s.search_paths(p, goals[20:], seed[20:], K, step, rng_seed=5, problem_offset=20)
        other = s.search_paths(p, goals[20:], seed[20:], K, step, rng_seed=5, problem_offset=0)
        same(whole, [np.concatenate([a, b]) for a, b in zip(lo, hi)], f"halves exact={exact}")
        assert not np.array_equal(other[0], hi[0])  # (the offset is what keys the restarts)
        # an invalid initial guess (a NaN, a variable outside its limits) is re-drawn at epoch 0
        guess = seed.copy()
        guess[::3, 1] = np.nan
        guess[1::3, 3] = ch.qmax[3] + 0.5
        got = s.search_paths(p, goals, seed, K, step, rng_seed=5, initial_guess=guess)
        want = SP.reference_search_paths(own_solve(s, p), ch, goals, seed, K, step, rng_seed=5, initial_guess=guess)
        same(got, want, f"invalid guesses exact={exact}")
    finally:
        s.close()


@pytest.mark.parametrize("limit", [None, 0.15])
def test_servo_mode_closes_at_attempt_0_unless_a_jump_is_refused(O, exact_flavour, limit):
    """return_approximate_solution = 1: every waypoint of an UNREACHABLE straight line returns the best configuration
    found (status APPROXIMATE), which is held -- only a refused jump reopens such a path"""
    ch = robots.panda()
    s = pk.Solver(ch, device=0, strict=True)
    try:
        with O.math_mode("portable"):
            _, goals, seed, K, _ = SP.fixture("panda", lambda c: O.Oracle(c).fk)
            goals[:, :, :3] += 2.0 * goals[:, :1, :3] / np.linalg.norm(goals[:, :1, :3], axis=2, keepdims=True)  # 2 m further out
            step = None if limit is None else np.full(ch.dof, limit)
            want = SP.oracle_search_paths(O, ch, goals, seed, K, step, kw=dict(return_approximate_solution=1),
                                          rng_seed=SP.RNG_SEED, trace=True)
        got = s.search_paths(pk.default_params(mode=1, return_approximate_solution=1), goals, seed, K, step, rng_seed=SP.RNG_SEED)
        same(got, want[:7], f"servo [{exact_flavour}] limit {limit}")
        sol, st, cost, stats, reached, attempts, totals = got
        W = goals.shape[1]
        assert not (st == pk.NO_IK_SOLUTION).any() and (st[st > 0] == pk.APPROXIMATE).all()
        if limit is None:
            assert (attempts == 1).all() and (reached == W).all()
        else:
            assert (want[7].jumped | (attempts == 1)).all()    # a path that ran again had a refused jump
            assert ((attempts == 1) == (want[7].reached[:, 0] == W)).all()
            assert (reached >= 1).all()                         # (waypoint 0 has no joint-step test)
            assert want[7].jumped.any()
    finally:
        s.close()


def test_device_entry_point_streams_and_slots():
    """search_paths_device on a non-default stream equals the host-pointer call; two slots in flight on two streams
    equal their serial answers (own interpreter: torch allocates the buffers)"""
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "startpath_device_check.py")], cwd=ROOT,
                       capture_output=True, text=True, timeout=900)
    assert r.returncode == 0 and "startpath device check OK" in r.stdout, r.stdout[-2000:] + r.stderr[-3000:]


def test_every_optional_array_may_be_absent(O):
    """P = 3 paths of W = 3 waypoints (odd row counts: the int32 arrays end off an 8-byte boundary): the call with
    every optional array, then with each one NULL in turn -- every array still given is the full call's, bit for bit
    (the initial guess given is the seed and the step limit "no limit": leaving them out changes no answer)"""
    ch = robots.panda()
    s = pk.Solver(ch, device=0)
    try:
        _, goals, seed, K, _ = SP.fixture("panda", lambda c: s.fk)
        goals, seed = np.ascontiguousarray(goals[5:8, :3]), np.ascontiguousarray(seed[5:8])
        p = pk.default_params(mode=1)
        full = A.check_optional_arrays(
            lambda a: raw_call(s._L, s._h, p, 3, 3, K, a, rng_seed=SP.RNG_SEED),
            lambda: fresh_arrays(s, goals, seed, seed.copy(), np.full(ch.dof, -1.0)),
            ("final_cost", "stats", "reached", "attempts", "totals", "initial_guess", "max_joint_step"), OUTPUTS)
        same([full[k] for k in OUTPUTS], s.search_paths(p, goals, seed, K, rng_seed=SP.RNG_SEED), "binding")
        assert (full["attempts"] > 1).any()  # (rows went through the slot's scratch)
    finally:
        s.close()


def test_edges_and_refusals(O):
    ch = robots.panda()
    s = pk.Solver(ch, device=0)
    L, h = s._L, s._h
    try:
        _, goals, seed, K, step = SP.fixture("panda", lambda c: s.fk)
        P, W = goals.shape[:2]
        p = pk.default_params(mode=1)
        ref = s.search_paths(p, goals, seed, K, step, rng_seed=SP.RNG_SEED)
        # no path: nothing to do
        e = s.search_paths(p, np.zeros((0, 5, 7)), np.zeros((0, 7)), 3)
        assert e[0].shape == (0, 5, 7) and e[1].shape == (0, 5) and e[4].shape == (0,) and e[6].shape == (0,)
        err = lambda: L.pikamd_last_error().decode()  # noqa: E731

        def raw(params, P_=P, W_=W, K_=K, **gone):
            a = fresh_arrays(s, goals, seed, None, step)
            a.update(gone)
            return raw_call(L, h, params, P_, W_, K_, a)

        assert raw(p) == 0
        # refusals: PIKAMD_EINVAL (-1) and a message
        assert raw(pk.default_params(mode=0)) == -1 and "local mode" in err()
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
        with pytest.raises(pk.PickIkAmdError, match="local mode"):
            s.search_paths(pk.default_params(), goals, seed, K)
        s.set_option("joint_layout", "soa")
        with pytest.raises(pk.PickIkAmdError, match="joint_layout soa"):
            s.search_paths(p, goals, seed, K)
        s.set_option("joint_layout", "aos")
        same(s.search_paths(p, goals, seed, K, step, rng_seed=SP.RNG_SEED), ref, "after the refusals")
    finally:
        s.close()


def test_cpp_host_mirror_search_paths():
    """tests/native/startpath_check.cpp: Solver::ik_gradient_search_paths against the C ABI call and, with one attempt,
    against the batch and path calls it is defined by"""
    import __graft_entry__ as g
    g.build()
    src = os.path.join(ROOT, "tests", "native", "startpath_check.cpp")
    exe = os.path.join(ROOT, "tests", "native", "startpath_check")
    lib_dir = os.path.join(ROOT, "pick_ik_amd")
    if not os.path.exists(exe) or os.path.getmtime(exe) < max(
            os.path.getmtime(src), os.path.getmtime(os.path.join(lib_dir, "host", "pick_ik_amd.hpp"))):
        subprocess.run(["g++", "-std=c++17", "-O1", "-pthread", "-Wall", "-Wextra", "-Werror", src, "-o", exe,
                        "-L" + lib_dir, "-lpick_ik_amd", "-Wl,-rpath," + lib_dir, "-Wl,-rpath,/opt/rocm/lib"], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "startpath C++ checks OK" in r.stdout, r.stdout + r.stderr


def test_one_call_beats_the_loop_of_round_trips(O):
    """The Panda fixture (48 straight lines of 6 waypoints from the home pose, up to 6 attempts, step limit 0.15; the
    default exact handle): one launch and two copies against the loop a caller writes today -- per attempt one
    solve_batch for waypoint 0 and one solve_paths for the rest, the closed paths taken out by hand, the restart states
    drawn ahead -- in the same process, both warmed, alternated 21 times, medians of a host clock around calls that end
    synchronised.  Both sides return the same `reached`, so they do the same work.  The baseline is existing, unchanged
    code and no margin is added.  (Figures of a run: profiles/startpath_latency.txt.)"""
    ch = robots.panda()
    s = pk.Solver(ch, device=0)
    try:
        _, goals, seed, K, step = SP.fixture("panda", lambda c: s.fk)
        p = pk.default_params(mode=1)
        table = SR.starts(ch, seed, K, SP.RNG_SEED)
        reached = s.search_paths(p, goals, seed, K, step, rng_seed=SP.RNG_SEED)[4]
        np.testing.assert_array_equal(reached, SP.host_loop(s, p, goals, seed, K, step, table))
        call, loop, _, _ = SP.time_call_against_loop(s, p, goals, seed, K, step, SP.RNG_SEED, table, reps=21)
        print(f"P = 48, W = 6, K = 6 [{s.search_paths_kernel_name(p, len(seed))}]: search_paths {call * 1e3:.3f} ms, "
              f"loop of solve_batch + solve_paths {loop * 1e3:.3f} ms, ratio {loop / call:.2f}")
        assert call < loop, (call, loop)
    finally:
        s.close()

