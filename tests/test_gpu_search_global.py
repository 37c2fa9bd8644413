"""Memetic IK with random restarts on the GPU (pikamd_search_global_batch): the loop searchPositionIK runs around the
solver, in global mode, for a batch, in one call.

Its result is DEFINED as the loop of one-record global-mode solves with rng_seed_a = rng_seed + (a << 32)
(include/pick_ik_amd.h; tests/search_global_reference.py holds that loop), so everything here compares at tolerance
zero: against the loop over the CPU oracle for the exact builds, against the loop over the handle's own solve_batches
for every flavour, every schedule against the others.  tests/test_search_global_cpu.py shows that the fixtures reach
every class (solved at the first attempt, later, never).  B = 64 problems of K = 4 attempts unless a test says
otherwise."""
import ctypes as C
import os
import subprocess
import sys
import time

import numpy as np
import pytest

import pick_ik_amd as pk
from tests import search_global_reference as GR
from tests import abi_calls as A
from tests import search_reference as SR

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ALL_NAMES = SR.NAMES + ("all_solution", "all_status")
B, K = 64, GR.K


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
    """the normative loop over the handle's own one-record solve_batches"""
    return GR.reference_search(GR.handle_solve_one(s, p), ch, goals, seed, k, **kw)


def handle_fixture(case, exact=None, strict=False, n=B, far=8, **more):
    s = pk.Solver(SR.CASES[case][0](), device=0, strict=strict, exact=exact)
    ch, goals, seed = GR.fixture(case, lambda _: s.fk, n, far)
    return s, ch, goals, seed, pk.default_params(mode=0, **GR.params_kw(case, **more))


@pytest.mark.parametrize("case", list(GR.GENERATIONS))
def test_search_equals_the_loop_over_the_oracle(O, exact_flavour, case):
    kw = GR.params_kw(case)
    with O.math_mode("portable"):
        ch, goals, seed = GR.fixture(case, lambda c: O.Oracle(c).fk, B)
        want = GR.oracle_search(O, ch, goals, seed, K, kw, rng_seed=GR.RNG_SEED)
    first, later, never = SR.search_counts(want[1], want[4])
    assert first >= 1 and later >= 1 and never >= 1, (case, exact_flavour, first, later, never)
    s = pk.Solver(ch, device=0, strict=True)
    try:
        p = pk.default_params(mode=0, **kw)
        got = s.search_global_batch(p, goals, seed, K, rng_seed=GR.RNG_SEED)
        print(f"{case} [{exact_flavour}] {s.kernel_name(p)}: first / later / never = {first}/{later}/{never}")
        same(got, want, f"{case} [{exact_flavour}]")
    finally:
        s.close()


@pytest.mark.parametrize("name,more", [("species", dict(memetic_num_threads=2)),
                                       ("elite_1", dict(memetic_elite_size=1, memetic_population_size=9)),
                                       ("approximate", dict(return_approximate_solution=1))])
def test_panda_variations_against_the_oracle(O, exact_flavour, name, more):
    kw = GR.params_kw("panda", **more)
    with O.math_mode("portable"):
        ch, goals, seed = GR.fixture("panda", lambda c: O.Oracle(c).fk, B)
        want = GR.oracle_search(O, ch, goals, seed, K, kw, rng_seed=GR.RNG_SEED)
    s = pk.Solver(ch, device=0, strict=True)
    try:
        got = s.search_global_batch(pk.default_params(mode=0, **kw), goals, seed, K, rng_seed=GR.RNG_SEED)
        same(got, want, f"{name} [{exact_flavour}]")
        first, later, never = SR.search_counts(got[1], got[4])
        if name == "approximate":
            assert (got[4] == 1).all() and (got[1] > 0).all()
        else:
            assert first >= 1 and later >= 1 and never >= 1, (name, first, later, never)
    finally:
        s.close()


@pytest.mark.parametrize("exact,case,namespaces", [
    (None, "panda", ("pik_exact", "pik_exact")),
    (False, "panda", ("pik_common", "pik_common_goals")),
    (False, "panda_unbounded", ("pik", "pik")),
    (None, "torso_dual_arm", ("pik_exact", "pik_exact")),
    (False, "torso_dual_arm", None),
], ids=["exact_panda", "fast_panda", "fast_unbounded", "exact_two_tips", "fast_two_tips"])
def test_search_equals_the_loop_over_the_handles_own_solves(O, exact, case, namespaces):
    s, ch, goals, seed, _ = handle_fixture(case, exact)
    try:
        for i, more in enumerate(({}, dict(minimal_displacement_weight=0.001))):
            p = pk.default_params(mode=0, **GR.params_kw(case, **more))
            if namespaces:
                assert s.kernel_name(p) == f"{namespaces[i]}::memetic_kernel<{ch.dof}>", s.kernel_name(p)
            want = own_loop(s, p, ch, goals, seed, K, rng_seed=3)
            got = s.search_global_batch(p, goals, seed, K, rng_seed=3)
            first, later, never = SR.search_counts(want[1], want[4])
            print(f"{case} exact={exact} {more} {s.kernel_name(p)}: first / later / never = {first}/{later}/{never}")
            same(got, want, f"{case} exact={exact} {more}")
            assert later >= 1 and never >= 1, (case, exact, more, first, later, never)
    finally:
        s.close()


def test_strict_library_against_its_own_solves(O):
    s, ch, goals, seed, p = handle_fixture("panda", strict=True)
    try:
        assert s.kernel_name(p) == "pik_strict::memetic_kernel<7>"
        same(s.search_global_batch(p, goals, seed, K, rng_seed=3), own_loop(s, p, ch, goals, seed, K, rng_seed=3), "strict")
    finally:
        s.close()


SCHEDULES = [("lanes_per_elite", v) for v in ("1", "2", "4", "8", "16")] + \
            [("passes", "none"), ("passes", "2,4,8"), ("two_per_simd", "2"), ("device_regime", "0"), ("device_regime", "1"),
             ("regime", "latency"), ("regime", "throughput")]


@pytest.mark.parametrize("exact", [None, False], ids=["default_exact", "fast"])
def test_schedules_change_no_bit(O, exact):
    s, ch, goals, seed, p = handle_fixture("panda", exact)
    try:
        ref = s.search_global_batch(p, goals, seed, K, rng_seed=1, all_attempts=True)
        plain = s.search_global_batch(p, goals, seed, K, rng_seed=1)
        same(plain, ref[:5], "without all_attempts")
        first, later, never = SR.search_counts(plain[1], plain[4])
        assert later >= 1 and never >= 1
        for name, value in SCHEDULES:
            s.set_option(name, value)
            same(s.search_global_batch(p, goals, seed, K, rng_seed=1), plain, f"{name} = {value}")
            same(s.search_global_batch(p, goals, seed, K, rng_seed=1, all_attempts=True), ref, f"{name} = {value} (all)")
            s.set_option(name, None)
        # park / resume inside a restart attempt, with every width
        s.set_option("passes", "2,4,8")
        for lanes in ("1", "4", "16"):
            s.set_option("lanes_per_elite", lanes)
            same(s.search_global_batch(p, goals, seed, K, rng_seed=1), plain, f"passes 2,4,8, lanes {lanes}")
        s.set_option("lanes_per_elite", None)
        s.set_option("passes", None)
        same(s.search_global_batch(p, goals, seed, K, rng_seed=1), plain, "options back at their defaults")
    finally:
        s.close()


@pytest.mark.parametrize("exact", [None, False], ids=["default_exact", "fast"])
def test_shapes(O, exact):
    """B in {1, 5, 64, 257} (257 does not fill its last wavefront) at K = 4, K in {1, 2, 64} at B = 5 with one target
    out of reach, against the loop over the handle's own solves"""
    s, ch, goals, seed, p = handle_fixture("panda", exact, n=257, far=0)
    goals[4, 0] += 5.0  # (within every B >= 5)
    goals[250:, 0] += 5.0
    try:
        for n, k in ((1, K), (5, K), (64, K), (257, K), (5, 1), (5, 2), (5, 64)):
            want = own_loop(s, p, ch, goals[:n], seed[:n], k, rng_seed=2)
            got = s.search_global_batch(p, goals[:n], seed[:n], k, rng_seed=2)
            same(got, want, f"B {n} K {k}")
            if n >= 5:
                assert got[4][4] == k and got[1][4] < 0
            if k == 1:  # one attempt from a valid start: exactly solve_batch
                same(got[:4], s.solve_batch(p, goals[:n], seed[:n], rng_seed=2), "K = 1")
                assert (got[4] == 1).all()
    finally:
        s.close()


@pytest.mark.parametrize("exact", [None, False], ids=["default_exact", "fast"])
def test_all_attempts_rows_are_single_solves(O, exact):
    """panda_unbounded: the kernels keep a stored population per problem -- a restarted problem must not read the
    previous attempt's"""
    s, ch, goals, seed, p = handle_fixture("panda_unbounded", exact)
    try:
        plain = s.search_global_batch(p, goals, seed, K, rng_seed=4, problem_offset=7)
        same(plain, own_loop(s, p, ch, goals, seed, K, rng_seed=4, problem_offset=7), "the loop")
        table = SR.starts(ch, seed, K, rng_seed=4, problem_offset=7)
        got = s.search_global_batch(p, goals, seed, K, rng_seed=4, problem_offset=7, all_attempts=True)
        same(got[:5], plain, "the primary outputs are unchanged by asking")
        for a in range(K):
            # (a batch keyed by problem_offset + b is its one-record solves)
            sol, st, _, _ = s.solve_batch(p, goals, seed, rng_seed=GR.attempt_seed(4, a), problem_offset=7,
                                          initial_guess=table[:, a])
            np.testing.assert_array_equal(got[5][:, a], sol, err_msg=f"row {a}: all_solution")
            np.testing.assert_array_equal(got[6][:, a], st, err_msg=f"row {a}: all_status")
            one = GR.handle_solve_one(s, p)(goals[5:6], seed[5:6], table[5:6, a], GR.attempt_seed(4, a), 7 + 5)
            np.testing.assert_array_equal(got[5][5, a], one[0][0])
        behind = np.arange(K)[None, :] >= plain[4][:, None]  # rows behind a problem's winner: real results
        assert behind.any() and (got[6][behind] > 0).any() and (got[6][behind] < 0).any()
    finally:
        s.close()


def test_invalid_initial_guesses(O, exact_flavour):
    """a third of the rows past a limit, one row NaN: their attempt 0 starts at draw(b, 0, .)"""
    kw = GR.params_kw("panda")
    with O.math_mode("portable"):
        ch, goals, seed = GR.fixture("panda", lambda c: O.Oracle(c).fk, B)
        guess = seed.copy()
        guess[::3, 1] = ch.qmax[1] + 0.25
        guess[1::6, 3] = ch.qmin[3] - 1.0e-9
        guess[7, 5] = np.nan
        want = GR.oracle_search(O, ch, goals, seed, K, kw, rng_seed=6, initial_guess=guess)
        valid_start = GR.oracle_search(O, ch, goals, seed, K, kw, rng_seed=6)
    assert not np.array_equal(want[0], valid_start[0])
    s = pk.Solver(ch, device=0, strict=True)
    try:
        got = s.search_global_batch(pk.default_params(mode=0, **kw), goals, seed, K, rng_seed=6, initial_guess=guess)
        same(got, want, f"invalid guesses [{exact_flavour}]")
        assert not np.isnan(got[0]).any()
    finally:
        s.close()


@pytest.mark.parametrize("exact", [None, False], ids=["default_exact", "fast"])
def test_shard_invariance_and_wide_seeds(O, exact):
    s, ch, goals, seed, p = handle_fixture("panda_unbounded", exact)
    try:
        for r in ((1 << 32) + 5, (0xffffffff << 32) + 5):  # (the second one wraps at attempt 1)
            whole = s.search_global_batch(p, goals, seed, K, rng_seed=r, problem_offset=1000, all_attempts=True)
            lo = s.search_global_batch(p, goals[:40], seed[:40], K, rng_seed=r, problem_offset=1000, all_attempts=True)
            hi = s.search_global_batch(p, goals[40:], seed[40:], K, rng_seed=r, problem_offset=1040, all_attempts=True)
            same([np.concatenate([a, b]) for a, b in zip(lo, hi)], whole, f"40 + 24, seed {r:#x}")
            same(whole[:5], own_loop(s, p, ch, goals, seed, K, rng_seed=r, problem_offset=1000), f"seed {r:#x}")
        assert GR.attempt_seed((0xffffffff << 32) + 5, 1) == 5
    finally:
        s.close()


def test_edges_and_refusals(O):
    s, ch, goals, seed, p = handle_fixture("panda", n=48)
    L, h = s._L, s._h
    try:
        ref = s.search_global_batch(p, goals, seed, K)
        e = s.search_global_batch(p, np.zeros((0, 7)), np.zeros((0, 7)), K, all_attempts=True)
        assert e[0].shape == (0, 7) and e[4].shape == (0,) and e[5].shape == (0, K, 7) and e[6].shape == (0, K)
        sol2, st2 = np.empty_like(ref[0]), np.empty_like(ref[1])
        dp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int32)

        def raw(params, n, k, goal=goals, seed_=seed, solution=sol2, status=st2):
            ptr = lambda a, t: None if a is None else a.ctypes.data_as(t)
            return L.pikamd_search_global_batch(h, C.byref(params), n, ptr(goal, dp), ptr(seed_, dp), None, C.c_uint64(0),
                                                0, k, ptr(solution, dp), ptr(status, ip), None, None, None, None, None)

        # the optional outputs may be NULL
        assert raw(p, len(seed), K) == 0
        np.testing.assert_array_equal(sol2, ref[0])
        np.testing.assert_array_equal(st2, ref[1])
        err = lambda: L.pikamd_last_error().decode()
        assert raw(pk.default_params(mode=1), len(seed), K) == -1 and "pikamd_search_batch" in err()
        for k in (0, -1, 65):
            assert raw(p, len(seed), k) == -1 and "max_attempts" in err(), k
        assert raw(p, -1, K) == -1 and "B >= 0" in err()
        for missing in ("goal", "seed_", "solution", "status"):
            assert raw(p, len(seed), K, **{missing: None}) == -1 and "must not be NULL" in err(), missing
        assert raw(p, 0, K, goal=None, seed_=None, solution=None, status=None) == 0
        none = [None] * 8
        dev = L.pikamd_search_global_batch_device
        assert dev(h, C.byref(p), 4, None, None, None, C.c_uint64(0), 0, K, *none, 0) == -1
        assert dev(h, C.byref(p), 0, None, None, None, C.c_uint64(0), 0, K, *none, 999) == -1 and "slot" in err()
        s.set_option("joint_layout", "soa")
        with pytest.raises(pk.PickIkAmdError, match="joint_layout soa"):
            s.search_global_batch(p, goals, seed, K)
        s.set_option("joint_layout", "aos")
        # pikamd_search_batch still refuses global mode
        with pytest.raises(pk.PickIkAmdError, match="local mode"):
            s.search_batch(p, goals, seed, K)
        same(s.search_global_batch(p, goals, seed, K), ref, "after the refusals")
        # ... and an ordinary solve on the same handle is what it was
        fresh = pk.Solver(ch, device=0)
        try:
            same(s.solve_batch(p, goals, seed, rng_seed=9), fresh.solve_batch(p, goals, seed, rng_seed=9), "solve_batch")
        finally:
            fresh.close()
    finally:
        s.close()


def test_every_optional_array_may_be_absent(O):
    """B = 3 problems of K = 3 attempts (odd row counts: the int32 arrays end off an 8-byte boundary): the call with
    every optional array, then with each one NULL in turn -- every array still given is the full call's, bit for bit"""
    s, ch, goals, seed, p = handle_fixture("panda", n=3, far=1)
    try:
        full = A.check_optional_arrays(
            lambda a: A.search(s._L, s._h, p, 3, 3, a, global_mode=True, rng_seed=3),
            lambda: A.search_arrays(s, goals, seed, seed.copy(), 3),
            ("final_cost", "stats", "attempts", "all_solution", "all_status", "initial_guess"),
            A.SEARCH_OUTPUTS)
        same([full[k] for k in A.SEARCH_OUTPUTS], s.search_global_batch(p, goals, seed, 3, rng_seed=3, all_attempts=True), "binding")
        assert full["attempts"][2] == 3 and full["status"][2] <= 0
    finally:
        s.close()


def test_device_entry_point_streams_and_slots():
    """search_global_batch_device on a non-default stream equals the host-pointer call; two slots in flight on two
    streams equal their serial answers; a larger, a smaller and the first call again on one slot (own interpreter:
    torch allocates the buffers)"""
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "search_global_device_check.py")], cwd=ROOT,
                       capture_output=True, text=True, timeout=900)
    assert r.returncode == 0 and "search global device check OK" in r.stdout, r.stdout[-2000:] + r.stderr[-3000:]


def test_cpp_host_mirror_search_global():
    """tests/native/search_global_check.cpp: Solver::ik_memetic_search_batch against the C ABI call"""
    import __graft_entry__ as g
    g.build()
    src = os.path.join(ROOT, "tests", "native", "search_global_check.cpp")
    exe = os.path.join(ROOT, "tests", "native", "search_global_check")
    lib_dir = os.path.join(ROOT, "pick_ik_amd")
    if not os.path.exists(exe) or os.path.getmtime(exe) < max(
            os.path.getmtime(src), os.path.getmtime(os.path.join(lib_dir, "host", "pick_ik_amd.hpp"))):
        subprocess.run(["g++", "-std=c++17", "-O1", "-pthread", "-Wall", "-Wextra", "-Werror", src, "-o", exe,
                        "-L" + lib_dir, "-lpick_ik_amd", "-Wl,-rpath," + lib_dir, "-Wl,-rpath,/opt/rocm/lib"], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "search global C++ checks OK" in r.stdout, r.stdout + r.stderr


def time_against_loop(s, p, ch, goals, seed, k, rng_seed=1, reps=5):
    """Wall-clock seconds of search_global_batch and of the hand-written host loop of solve_batches round trips on the
    same problems (failures compacted by hand, its restart states drawn ahead, outside the clock): both warmed, then
    alternated `reps` times, a host clock around calls that end synchronised.  Returns (median call, median loop)."""
    table = SR.starts(ch, seed, k, rng_seed=rng_seed)
    for _ in range(2):
        s.search_global_batch(p, goals, seed, k, rng_seed=rng_seed)
        GR.host_loop(s, p, goals, seed, k, rng_seed, table)
    tc, tl = [], []
    for _ in range(reps):
        t0 = time.perf_counter()
        s.search_global_batch(p, goals, seed, k, rng_seed=rng_seed)
        t1 = time.perf_counter()
        GR.host_loop(s, p, goals, seed, k, rng_seed, table)
        t2 = time.perf_counter()
        tc.append(t1 - t0)
        tl.append(t2 - t1)
    return float(np.median(tc)), float(np.median(tl))


def test_one_call_is_not_slower_than_the_loop_of_round_trips(O):
    """(a) B = 4096, K = 4, defaults except memetic_max_generations = 16 (a few per cent fail) and (b) B = 1, K = 16
    with the target out of reach; Panda, the default exact handle.  One call against the host loop of solve_batches
    round trips on the same handle -- what a caller writes without this entry point.  Interleaved, median of five; the
    call may take at most 1.1 x the loop's time (the run-to-run spread an interleaved A/B resolves).  Measured figures:
    DESIGN.md section 6."""
    s = pk.Solver(SR.CASES["panda"][0](), device=0)
    try:
        ch, goals, seed, _ = SR.fixture("panda", lambda _: s.fk, 4096)
        p = pk.default_params(mode=0, memetic_max_generations=16)
        call, loop = time_against_loop(s, p, ch, goals, seed, K)
        got = s.search_global_batch(p, goals, seed, K, rng_seed=1)
        print(f"(a) B = 4096, K = {K}: search_global_batch {call * 1e3:.3f} ms, loop of solve_batches {loop * 1e3:.3f} ms, "
              f"ratio {loop / call:.2f}; first / later / never = {SR.search_counts(got[1], got[4])}")
        far = goals[:1].copy()
        far[0, 0] += 5.0
        call1, loop1 = time_against_loop(s, p, ch, far, seed[:1], 16)
        assert s.search_global_batch(p, far, seed[:1], 16, rng_seed=1)[4][0] == 16
        print(f"(b) B = 1, K = 16: search_global_batch {call1 * 1e3:.3f} ms, loop of solve_batches {loop1 * 1e3:.3f} ms, "
              f"ratio {loop1 / call1:.2f}")
        assert call <= 1.1 * loop, (call, loop)
        assert call1 <= 1.1 * loop1, (call1, loop1)
    finally:
        s.close()
