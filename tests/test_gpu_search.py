"""Local IK with random restarts on the GPU (pikamd_search_batch): the loop searchPositionIK runs around the solver, for
a batch, in one launch.

Its result is DEFINED as what the loop of local-mode solve_batch calls returns (include/pick_ik_amd.h;
tests/search_reference.py holds that loop and the restart draw in numpy), so everything here compares at tolerance
zero: against the loop over the CPU oracle for the exact builds, against the loop over the handle's own solve_batch
for the fast flavour, every kernel variant and both schedules against each other.  tests/test_search_cpu.py shows that
the fixtures reach every class (solved at the first attempt, later, never).  B = 64 problems of K = 4 attempts unless
a test says otherwise."""
import ctypes as C
import os
import subprocess
import sys
import time

import numpy as np
import pytest

import pick_ik_amd as pk
from tests import abi_calls as A
from tests import search_reference as SR

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ALL_NAMES = SR.NAMES + ("all_solution", "all_status")
B, K = 64, 4


@pytest.fixture(scope="module")
def O(oracle_mod):
    import __graft_entry__ as g
    g.build()
    return oracle_mod


def same(a, b, what=""):
    assert len(a) == len(b), what
    for x, y, w in zip(a, b, ALL_NAMES):
        np.testing.assert_array_equal(x, y, err_msg=f"{what}: {w}")


def own_loop(s, p, ch, goals, seed, k, **kw):
    """the normative loop over the handle's own solve_batch"""
    return SR.reference_search(lambda g, sd, ig: s.solve_batch(p, g, sd, initial_guess=ig), ch, goals, seed, k, **kw)


def handle_fixture(case, exact=None, strict=False, n=B):
    s = pk.Solver(SR.CASES[case][0](), device=0, strict=strict, exact=exact)
    ch, goals, seed, kw = SR.fixture(case, lambda _: s.fk, n)
    return s, ch, goals, seed, pk.default_params(mode=1, **kw)


@pytest.mark.parametrize("case", list(SR.CASES))
def test_search_equals_the_loop_over_the_oracle(O, exact_flavour, case):
    with O.math_mode("portable"):
        ch, goals, seed, kw = SR.fixture(case, lambda c: O.Oracle(c).fk, B)
        want = SR.oracle_search(O, ch, goals, seed, K, kw, rng_seed=SR.RNG_SEED)
    first, later, never = SR.search_counts(want[1], want[4])
    assert first >= 1 and later >= 1 and never >= 1, (case, exact_flavour, first, later, never)
    s = pk.Solver(ch, device=0, strict=True)
    try:
        p = pk.default_params(mode=1, **kw)
        got = s.search_batch(p, goals, seed, K, rng_seed=SR.RNG_SEED)
        print(f"{case} [{exact_flavour}] {s.search_kernel_name(p, B, K)}: first / later / never = {first}/{later}/{never}")
        same(got, want, f"{case} [{exact_flavour}]")
    finally:
        s.close()


@pytest.mark.parametrize("exact", [None, False], ids=["default_exact", "fast"])
@pytest.mark.parametrize("case", ["panda", "torso_dual_arm"])
def test_search_equals_the_loop_over_the_handles_own_solve_batch(O, case, exact):
    s, ch, goals, seed, _ = handle_fixture(case, exact)
    try:
        for kw in ({}, dict(minimal_displacement_weight=0.001)):
            p = pk.default_params(mode=1, **kw)
            want = own_loop(s, p, ch, goals, seed, K, rng_seed=3)
            got = s.search_batch(p, goals, seed, K, rng_seed=3)
            first, later, never = SR.search_counts(want[1], want[4])
            print(f"{case} exact={exact} {kw}: first / later / never = {first}/{later}/{never}")
            same(got, want, f"{case} exact={exact} {kw}")
            assert first >= 1 and later >= 1, (case, exact, kw, first, later, never)  # (a restart was needed and won)
    finally:
        s.close()


def variant_sweep(s, ch, goals, seed, p, lanes, served=True):
    """every forced width in both schedules against the adaptive choice, with the kernel each call reports"""
    ref = s.search_batch(p, goals, seed, K, rng_seed=1, all_attempts=True)
    plain = s.search_batch(p, goals, seed, K, rng_seed=1)
    same(plain, ref[:5], "without all_attempts")
    assert s.self_test(p, 32) == 0  # (no width switched off on this chain: a forced width is the width that runs)
    for l, name in lanes.items():
        s.set_option("lanes_per_elite", l)
        for schedule, in_flight in (("sequential", 1), ("parallel", K)):
            s.set_option("search_schedule", schedule)
            assert s.search_kernel_name(p, B, K) == (name if served else lanes[1], in_flight), (l, schedule)
            same(s.search_batch(p, goals, seed, K, rng_seed=1, all_attempts=True), ref, f"lanes {l} {schedule} (all)")
            same(s.search_batch(p, goals, seed, K, rng_seed=1), plain, f"lanes {l} {schedule}")
    s.set_option("lanes_per_elite", None)
    s.set_option("search_schedule", None)
    return ref


@pytest.mark.parametrize("exact,case,lanes", [
    (None, "panda", {1: "pik_exact::ik_search_kernel<7,false>", 4: "pik_exact::ik_search_team_kernel<7,4>",
                     16: "pik_exact::ik_search_team_kernel<7,16>"}),
    (False, "panda", {1: "pik::ik_search_kernel<7,false>", 8: "pik::ik_search_wide_kernel<7,8,false>",
                      16: "pik::ik_search_wide_kernel<7,16,false>"}),
    (False, "torso_dual_arm", {1: "pik::ik_search_kernel<9,true>", 8: "pik::ik_search_wide_kernel<9,8,true>",
                               16: "pik::ik_search_wide_kernel<9,16,true>"}),
    # (exact flavours, several tips: one lane per unit whatever is asked for)
    (None, "torso_dual_arm", {1: "pik_exact::ik_search_kernel<9,true>", 16: "pik_exact::ik_search_kernel<9,true>"}),
], ids=["exact_panda", "fast_panda", "fast_two_tips", "exact_two_tips"])
def test_every_variant_returns_the_same_bits(O, exact, case, lanes):
    s, ch, goals, seed, _ = handle_fixture(case, exact)
    try:
        p = pk.default_params(mode=1, minimal_displacement_weight=0.001)
        # (the cooperative kernels for several tips serve chains whose tips are all plain Denavit-Hartenberg ones: a
        #  handle they do not serve runs one lane per unit whatever is asked for, and says so)
        served = case == "panda" or exact is not False or "ik_search_wide_kernel" in s.search_kernel_name(p, 1, 1)[0]
        variant_sweep(s, ch, goals, seed, p, lanes, served)
        # the adaptive rule: one plugin-style query with 16 attempts has them all in flight, on the widest kernel ...
        name, in_flight = s.search_kernel_name(p, 1, 16)
        assert in_flight == 16
        if case == "panda":
            assert name.endswith(",16>") or ",16," in name, name
        # ... one attempt has nothing to run side by side, and a call far too large walks its attempts, one lane each
        assert s.search_kernel_name(p, 1, 1)[1] == 1
        name, in_flight = s.search_kernel_name(p, 1 << 20, K)
        assert in_flight == 1 and "ik_search_kernel<" in name
    finally:
        s.close()


def test_strict_library_variants(O):
    s, ch, goals, seed, p = handle_fixture("panda", strict=True)
    try:
        variant_sweep(s, ch, goals, seed, p,
                      {1: "pik_strict::ik_search_kernel<7,false>", 4: "pik_strict::ik_search_team_kernel<7,4>",
                       16: "pik_strict::ik_search_team_kernel<7,16>"})
    finally:
        s.close()


@pytest.mark.parametrize("exact", [None, False], ids=["default_exact", "fast"])
def test_shapes(O, exact):
    """B in {1, 5, 64, 257} (257 does not fill its last wavefront) at K = 4, K in {1, 2, 64} at B = 5, in both
    schedules and the adaptive one, against the loop over the handle's own solve_batch"""
    s, ch, goals, seed, p = handle_fixture("panda", exact, n=257)
    try:
        for n, k in ((1, K), (5, K), (64, K), (257, K), (5, 1), (5, 2), (5, 64)):
            want = own_loop(s, p, ch, goals[:n], seed[:n], k, rng_seed=2)
            for schedule in (None, "sequential", "parallel"):
                s.set_option("search_schedule", schedule)
                same(s.search_batch(p, goals[:n], seed[:n], k, rng_seed=2), want, f"B {n} K {k} {schedule}")
            if k == 1:  # one attempt from a valid start: exactly solve_batch
                same(want[:4], s.solve_batch(p, goals[:n], seed[:n]), "K = 1")
                assert (want[4] == 1).all()
    finally:
        s.close()


@pytest.mark.parametrize("exact", [None, False], ids=["default_exact", "fast"])
def test_all_attempts_rows_are_single_solves(O, exact):
    s, ch, goals, seed, p = handle_fixture("panda_unbounded", exact)
    try:
        plain = s.search_batch(p, goals, seed, K, rng_seed=4)
        table = SR.starts(ch, seed, K, rng_seed=4)
        for schedule in ("sequential", "parallel"):
            s.set_option("search_schedule", schedule)
            got = s.search_batch(p, goals, seed, K, rng_seed=4, all_attempts=True)
            same(got[:5], plain, f"{schedule}: the primary outputs are unchanged by asking")
            for a in range(K):
                sol, st, _, _ = s.solve_batch(p, goals, seed, initial_guess=table[:, a])
                np.testing.assert_array_equal(got[5][:, a], sol, err_msg=f"{schedule} row {a}: all_solution")
                np.testing.assert_array_equal(got[6][:, a], st, err_msg=f"{schedule} row {a}: all_status")
        behind = np.arange(K)[None, :] >= plain[4][:, None]  # rows behind a problem's winner: real results
        assert behind.any() and (got[6][behind] > 0).any() and (got[6][behind] < 0).any()
    finally:
        s.close()


def test_invalid_initial_guesses(O, exact_flavour):
    """a third of the rows past a limit, one row NaN: their attempt 0 starts at draw(b, 0, .)"""
    with O.math_mode("portable"):
        ch, goals, seed, kw = SR.fixture("panda", lambda c: O.Oracle(c).fk, B)
        guess = seed.copy()
        guess[::3, 1] = ch.qmax[1] + 0.25
        guess[1::6, 3] = ch.qmin[3] - 1.0e-9
        guess[7, 5] = np.nan
        want = SR.oracle_search(O, ch, goals, seed, K, kw, rng_seed=6, initial_guess=guess)
        valid_start = SR.oracle_search(O, ch, goals, seed, K, kw, rng_seed=6)
    assert not np.array_equal(want[0], valid_start[0])
    s = pk.Solver(ch, device=0, strict=True)
    try:
        for schedule in ("sequential", "parallel"):
            s.set_option("search_schedule", schedule)
            got = s.search_batch(pk.default_params(mode=1), goals, seed, K, rng_seed=6, initial_guess=guess)
            same(got, want, f"invalid guesses [{exact_flavour}] {schedule}")
        assert not np.isnan(got[0]).any()
    finally:
        s.close()


@pytest.mark.parametrize("exact", [None, False], ids=["default_exact", "fast"])
def test_shard_invariance_and_wide_seeds(O, exact):
    s, ch, goals, seed, p = handle_fixture("panda_unbounded", exact)
    try:
        r1, r2 = (1 << 32) + 5, (2 << 32) + 5  # (equal low words: the high word of the seed is in the key)
        whole = s.search_batch(p, goals, seed, K, rng_seed=r1, problem_offset=1000, all_attempts=True)
        lo = s.search_batch(p, goals[:40], seed[:40], K, rng_seed=r1, problem_offset=1000, all_attempts=True)
        hi = s.search_batch(p, goals[40:], seed[40:], K, rng_seed=r1, problem_offset=1040, all_attempts=True)
        same([np.concatenate([a, b]) for a, b in zip(lo, hi)], whole, "40 + 24")
        same(whole[:5], own_loop(s, p, ch, goals, seed, K, rng_seed=r1, problem_offset=1000), "offset 1000")
        other = s.search_batch(p, goals, seed, K, rng_seed=r2, problem_offset=1000, all_attempts=True)
        np.testing.assert_array_equal(other[5][:, 0], whole[5][:, 0])  # (attempt 0 draws nothing)
        assert not np.array_equal(other[5][:, 1:], whole[5][:, 1:])
        same(other[:5], own_loop(s, p, ch, goals, seed, K, rng_seed=r2, problem_offset=1000), "second seed")
    finally:
        s.close()


def test_approximate_mode_closes_every_problem_at_once(O, exact_flavour):
    with O.math_mode("portable"):
        ch, goals, seed, kw = SR.fixture("panda", lambda c: O.Oracle(c).fk, B)
        want = SR.oracle_search(O, ch, goals, seed, K, dict(return_approximate_solution=1))
    s = pk.Solver(ch, device=0, strict=True)
    try:
        for schedule in ("sequential", "parallel"):
            s.set_option("search_schedule", schedule)
            got = s.search_batch(pk.default_params(mode=1, return_approximate_solution=1), goals, seed, K)
            same(got, want, f"approximate [{exact_flavour}] {schedule}")
        assert (got[4] == 1).all() and (got[1] > 0).all() and (got[1] == pk.APPROXIMATE).any()
    finally:
        s.close()


def test_edges_and_refusals(O):
    s, ch, goals, seed, p = handle_fixture("panda", n=48)
    L, h = s._L, s._h
    try:
        ref = s.search_batch(p, goals, seed, K)
        # no problem: nothing to do
        e = s.search_batch(p, np.zeros((0, 7)), np.zeros((0, 7)), K, all_attempts=True)
        assert e[0].shape == (0, 7) and e[4].shape == (0,) and e[5].shape == (0, K, 7) and e[6].shape == (0, K)
        # the optional outputs may be NULL
        sol2, st2 = np.empty_like(ref[0]), np.empty_like(ref[1])
        dp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int32)

        def raw(params, n, k, goal=goals, seed_=seed, solution=sol2, status=st2):
            ptr = lambda a, t: None if a is None else a.ctypes.data_as(t)
            return L.pikamd_search_batch(h, C.byref(params), n, ptr(goal, dp), ptr(seed_, dp), None, C.c_uint64(0), 0, k,
                                         ptr(solution, dp), ptr(status, ip), None, None, None, None, None)

        assert raw(p, len(seed), K) == 0
        np.testing.assert_array_equal(sol2, ref[0])
        np.testing.assert_array_equal(st2, ref[1])
        # refusals: PIKAMD_EINVAL (-1) and a message
        err = lambda: L.pikamd_last_error().decode()
        assert raw(pk.default_params(mode=0), len(seed), K) == -1 and "local mode" in err() and "memetic" in err()
        for k in (0, -1, 65):
            assert raw(p, len(seed), k) == -1 and "max_attempts" in err(), k
        assert raw(p, len(seed), 64) == 0
        assert raw(p, -1, K) == -1 and "B >= 0" in err()
        for missing in ("goal", "seed_", "solution", "status"):
            assert raw(p, len(seed), K, **{missing: None}) == -1 and "must not be NULL" in err(), missing
        assert raw(p, 0, K, goal=None, seed_=None, solution=None, status=None) == 0
        none = [None] * 8
        assert L.pikamd_search_batch_device(h, C.byref(p), 4, None, None, None, C.c_uint64(0), 0, K, *none, 0) == -1
        assert L.pikamd_search_batch_device(h, C.byref(p), 0, None, None, None, C.c_uint64(0), 0, K, *none, 999) == -1
        assert "slot" in err()
        with pytest.raises(pk.PickIkAmdError, match="local mode"):
            s.search_batch(pk.default_params(), goals, seed, K)
        with pytest.raises(pk.PickIkAmdError, match="search_schedule"):
            s.set_option("search_schedule", "sideways")
        s.set_option("joint_layout", "soa")
        with pytest.raises(pk.PickIkAmdError, match="joint_layout soa"):
            s.search_batch(p, goals, seed, K)
        s.set_option("joint_layout", "aos")
        same(s.search_batch(p, goals, seed, K), ref, "after the refusals")
    finally:
        s.close()


def test_every_optional_array_may_be_absent(O):
    """B = 3 problems of K = 3 attempts (odd row counts: the int32 arrays end off an 8-byte boundary): the call with
    every optional array, then with each one NULL in turn -- every array still given is the full call's, bit for bit"""
    s = pk.Solver(SR.CASES["panda"][0](), device=0)
    try:
        ch, goals, seed, _ = SR.fixture("panda", lambda _: s.fk, 3)
        goals[2, 0] += 5.0  # (out of reach: every attempt of this problem runs)
        p = pk.default_params(mode=1)
        full = A.check_optional_arrays(
            lambda a: A.search(s._L, s._h, p, 3, 3, a, rng_seed=3), lambda: A.search_arrays(s, goals, seed, seed.copy(), 3),
            ("final_cost", "stats", "attempts", "all_solution", "all_status", "initial_guess"),
            A.SEARCH_OUTPUTS)
        same([full[k] for k in A.SEARCH_OUTPUTS], s.search_batch(p, goals, seed, 3, rng_seed=3, all_attempts=True), "binding")
        assert full["attempts"][2] == 3 and full["status"][2] <= 0
    finally:
        s.close()


def test_device_entry_point_streams_and_slots():
    """search_batch_device on a non-default stream equals the host-pointer call; two slots in flight on two streams
    equal their serial answers (own interpreter: torch allocates the buffers)"""
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "search_device_check.py")], cwd=ROOT,
                       capture_output=True, text=True, timeout=900)
    assert r.returncode == 0 and "search device check OK" in r.stdout, r.stdout[-2000:] + r.stderr[-3000:]


def test_cpp_host_mirror_search():
    """tests/native/search_check.cpp: Solver::ik_gradient_search_batch against the C ABI call and ik_gradient_batch"""
    import __graft_entry__ as g
    g.build()
    src = os.path.join(ROOT, "tests", "native", "search_check.cpp")
    exe = os.path.join(ROOT, "tests", "native", "search_check")
    lib_dir = os.path.join(ROOT, "pick_ik_amd")
    if not os.path.exists(exe) or os.path.getmtime(exe) < max(
            os.path.getmtime(src), os.path.getmtime(os.path.join(lib_dir, "host", "pick_ik_amd.hpp"))):
        subprocess.run(["g++", "-std=c++17", "-O1", "-pthread", "-Wall", "-Wextra", "-Werror", src, "-o", exe,
                        "-L" + lib_dir, "-lpick_ik_amd", "-Wl,-rpath," + lib_dir, "-Wl,-rpath,/opt/rocm/lib"], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "search C++ checks OK" in r.stdout, r.stdout + r.stderr


def time_against_loop(s, p, ch, goals, seed, k, reps=21):
    """Wall-clock seconds of search_batch and of the hand-written host loop of solve_batch round trips on the same
    problems (its restart states drawn ahead, outside the clock): both warmed, then alternated `reps` times, a host
    clock around calls that end synchronised.  Returns (median call, median loop)."""
    table = SR.starts(ch, seed, k)
    for _ in range(2):
        got = s.search_batch(p, goals, seed, k)
        st, att = SR.host_loop(s, p, goals, seed, k, start_table=table)
        np.testing.assert_array_equal(got[1], st)
        np.testing.assert_array_equal(got[4], att)
    tc, tl = [], []
    for _ in range(reps):
        t0 = time.perf_counter()
        s.search_batch(p, goals, seed, k)
        t1 = time.perf_counter()
        SR.host_loop(s, p, goals, seed, k, start_table=table)
        t2 = time.perf_counter()
        tc.append(t1 - t0)
        tl.append(t2 - t1)
    return float(np.median(tc)), float(np.median(tl))


def test_one_call_beats_the_loop_of_round_trips(O):
    """(a) B = 4096, K = 4 and (b) B = 1, K = 16 with a target out of reach, so that every attempt runs; Panda, the
    default exact handle.  One call against the host loop of solve_batch round trips on the same handle -- what a
    caller wrote before this entry point existed.  The loop pays K round trips where the call pays one: the assertion
    is t_call < t_loop, no margin fixed in advance.  Measured figures: DESIGN.md section 6."""
    s, ch, goals, seed, p = handle_fixture("panda", n=4096)
    try:
        call, loop = time_against_loop(s, p, ch, goals, seed, K)
        print(f"(a) B = 4096, K = {K} [{s.search_kernel_name(p, 4096, K)}]: search_batch {call * 1e3:.3f} ms, loop of "
              f"solve_batch {loop * 1e3:.3f} ms, ratio {loop / call:.2f}")
        far = goals[:1].copy()
        far[0, :3] = [3.0, 0.0, 0.5]  # three metres out: no attempt can succeed
        call1, loop1 = time_against_loop(s, p, ch, far, seed[:1], 16)
        assert s.search_batch(p, far, seed[:1], 16)[4][0] == 16
        print(f"(b) B = 1, K = 16 [{s.search_kernel_name(p, 1, 16)}]: search_batch {call1 * 1e3:.3f} ms, loop of "
              f"solve_batch {loop1 * 1e3:.3f} ms, ratio {loop1 / call1:.2f}")
        assert call < loop, (call, loop)
        assert call1 < loop1, (call1, loop1)
    finally:
        s.close()
