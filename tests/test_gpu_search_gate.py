"""The approximate-solution gate inside the restart searches, on the GPU (pikamd_gate_batch,
pikamd_set_approximate_gate): with return_approximate_solution set, pikamd_search_batch and pikamd_search_global_batch
pass every answer through the reference's gate (src/pick_ik_plugin.cpp:219-267) and restart on a refusal.

Everything compares at tolerance zero against tests/gate_reference.py: the gated loop over the CPU oracle for the
exact builds, the gated loop over the handle's own solve_batch + gate -- the definition -- for every flavour.
tests/test_gate_cpu.py shows that the `panda` fixture reaches every class.  B = 64 problems of 8 attempts unless a test
says otherwise; every case below has answers accepted at once and answers never accepted under the oracle, all but `rr`
also answers accepted at a later attempt (asserted where the reference is the oracle's)."""
import os

import numpy as np
import pytest

import pick_ik_amd as pk
from tests import gate_reference as GT
from tests import search_reference as SR

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ALL_NAMES = SR.NAMES + ("all_solution", "all_status")
B, K = 64, GT.K
GATE = GT.PANDA_GATE
CASES = ("rr", "panda", "panda_on_torso", "torso_dual_arm", "floating_panda_fixed_base", "panda_unbounded")


@pytest.fixture(scope="module")
def O(oracle_mod):
    import __graft_entry__ as g
    g.build()
    return oracle_mod


def same(a, b, what=""):
    assert len(a) == len(b), what
    for x, y, w in zip(a, b, ALL_NAMES):
        np.testing.assert_array_equal(x, y, err_msg=f"{what}: {w}")


def case_kw(case):
    return dict(SR.CASES[case][3], **GT.PANDA_KW)


def handle_fixture(case, exact=None, n=B):
    s = pk.Solver(SR.CASES[case][0](), device=0, exact=exact)
    ch, goals, seed, _ = SR.fixture(case, lambda _: s.fk, n)
    return s, ch, goals, seed, pk.default_params(mode=1, **case_kw(case))


def set_gate(s, gate):
    if gate is None:
        s.clear_approximate_gate()
    else:
        s.set_approximate_gate(gate.cost_threshold, gate.joint_threshold)


def candidates(s, p, goals, seed):
    """joint vectors for the gate: what a solve returns (either status), and the same moved off by up to 3 rad in one
    variable, so that the joint limit has work on both sides of 2.5"""
    sol = s.solve_batch(p, goals, seed)[0]
    far = sol.copy()
    far[:, 0] += np.linspace(-3.0, 3.0, len(far))
    return np.concatenate([sol, far]), np.concatenate([goals, goals]), np.concatenate([seed, seed])


GATES = (GATE, GT.Gate(0.0, 0.0), GT.Gate(6e-4, 0.0), GT.Gate(0.0, 2.5), GT.Gate(1e-3, float("nan")), GT.Gate(-1.0, -1.0))


@pytest.mark.parametrize("case,n", [("panda", 64), ("torso_dual_arm", 32)])
def test_gate_is_cost_under_the_gates_parameters_and_the_joint_test(O, exact_flavour, case, n):
    """Solver.gate against the composition the header defines it by, on the same handle, and against the oracle"""
    with O.math_mode("portable"):
        ch, goals, seed, _ = SR.fixture(case, lambda c: O.Oracle(c).fk, n)
        s = pk.Solver(ch, device=0, strict=True)
        try:
            p = pk.default_params(mode=1, **case_kw(case))
            q, g2, sd2 = candidates(s, p, goals, seed)
            o = O.Oracle(ch)
            po = O.default_params(mode=1, **case_kw(case))
            seen = set()
            for gate in GATES:
                got = s.gate(p, GT.handle_gate(gate), g2, sd2, q)
                own = GT.gate_pass(s.cost, p, gate, g2, sd2, q)
                want = GT.gate_pass(GT.oracle_cost(o), po, gate, g2, sd2, q)
                np.testing.assert_array_equal(got, own, err_msg=f"{case} {gate}: cost + joint test on the handle")
                np.testing.assert_array_equal(got, want, err_msg=f"{case} {gate}: the oracle")
                seen |= set(got.tolist())
            assert seen == {True, False}
            within = GT.joint_test(GATE, sd2, q)
            assert within.any() and (~within).any()  # (the joint limit has candidates on both sides)
            assert s.gate(p, GT.handle_gate(GATE), goals[:0], seed[:0], seed[:0]).shape == (0,)
        finally:
            s.close()


@pytest.mark.parametrize("exact", [None, False], ids=["default_exact", "fast"])
def test_gate_on_the_fast_flavour_and_refusals(O, exact):
    s, ch, goals, seed, p = handle_fixture("panda", exact)
    try:
        q, g2, sd2 = candidates(s, p, goals, seed)
        for gate in GATES:
            np.testing.assert_array_equal(s.gate(p, GT.handle_gate(gate), g2, sd2, q),
                                          GT.gate_pass(s.cost, p, gate, g2, sd2, q), err_msg=str(gate))
        import ctypes as C
        L, h = s._L, s._h
        dp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int32)
        out = np.zeros(len(q), dtype=np.int32)
        gate = pk.Gate(6e-4, 2.5)
        args = dict(gate=C.byref(gate), goal=g2.ctypes.data_as(dp), seed=sd2.ctypes.data_as(dp), q=q.ctypes.data_as(dp),
                    out=out.ctypes.data_as(ip))
        call = lambda a, n=len(q): L.pikamd_gate_batch(h, C.byref(p), a["gate"], n, a["goal"], a["seed"], a["q"], a["out"])
        assert call(args) == 0
        for missing in args:
            assert call(dict(args, **{missing: None})) == -1 and "must not be NULL" in L.pikamd_last_error().decode(), missing
        assert call(args, 0) == 0 and call(args, -1) == -1
        s.set_option("joint_layout", "soa")
        assert call(args) == -1 and "joint_layout soa" in L.pikamd_last_error().decode()
        s.set_option("joint_layout", "aos")
        assert call(args) == 0
    finally:
        s.close()


_oracle_cache = {}


def oracle_reference(O, flavour, case, n, all_attempts):
    """the gated loop over the CPU oracle, computed once per (exact build, case, size)"""
    key = (flavour, case, n)
    if key not in _oracle_cache:
        ch, goals, seed, _ = SR.fixture(case, lambda c: O.Oracle(c).fk, n)
        every = GT.oracle_search(O, ch, goals, seed, K, case_kw(case), GATE, rng_seed=SR.RNG_SEED, all_attempts=True)
        for a in every:
            a.setflags(write=False)
        _oracle_cache[key] = (ch, goals, seed, every)
    ch, goals, seed, every = _oracle_cache[key]
    return ch, goals, seed, (every if all_attempts else every[:5])


def sweep_against_oracle(O, flavour, case, n, lanes=(1, 4, 16), schedules=("sequential", "parallel", "adaptive")):
    with O.math_mode("portable"):
        ch, goals, seed, want = oracle_reference(O, flavour, case, n, True)
    first, later, never = SR.search_counts(want[1], want[4])
    assert first >= 1 and never >= 1 and (later >= 1 or case == "rr"), (case, first, later, never)
    assert (want[6] == GT.GATE_REFUSED).any() and (want[6] > 0).any()
    s = pk.Solver(ch, device=0, strict=True)
    try:
        p = pk.default_params(mode=1, **case_kw(case))
        set_gate(s, GATE)
        names = set()
        for l in lanes:
            s.set_option("lanes_per_elite", l)
            for schedule in schedules:
                s.set_option("search_schedule", schedule)
                names.add(s.search_kernel_name(p, n, K))
                what = f"{case} [{flavour}] B {n} lanes {l} {schedule}"
                same(s.search_batch(p, goals, seed, K, rng_seed=SR.RNG_SEED, all_attempts=True), want, what + " (all)")
                same(s.search_batch(p, goals, seed, K, rng_seed=SR.RNG_SEED), want[:5], what)
        print(f"{case} [{flavour}] B {n}: first / later / never = {first}/{later}/{never}; kernels {sorted(names)}")
        return names
    finally:
        s.close()


@pytest.mark.parametrize("case", CASES)
def test_gated_search_equals_the_gated_loop_over_the_oracle(O, exact_flavour, case):
    """every schedule x 1 / 4 / 16 lanes per unit, with and without all_*"""
    names = sweep_against_oracle(O, exact_flavour, case, B)
    if case in ("rr", "panda", "panda_unbounded"):  # (one tip frame, no floating joint: the team kernels serve it)
        assert any("team_kernel" in n and n.endswith(",4>") for n, _ in names), names
        assert any("team_kernel" in n and n.endswith(",16>") for n, _ in names), names
    assert {k for _, k in names} == {1, K}  # (both schedules ran)


def test_gated_search_with_a_ragged_last_wavefront(O, exact_flavour):
    sweep_against_oracle(O, exact_flavour, "panda", 70)


@pytest.mark.parametrize("exact", [None, False], ids=["default_exact", "fast"])
@pytest.mark.parametrize("case", ["panda", "torso_dual_arm"])
def test_gated_search_equals_the_gated_loop_over_the_handle(O, case, exact):
    """the definition: solve_batch + gate on the same handle, attempt by attempt -- for the fast flavour too"""
    s, ch, goals, seed, p = handle_fixture(case, exact)
    try:
        for gate in (GATE, GT.Gate(0.0, 0.0)):
            set_gate(s, None)
            want = GT.handle_search(s, p, gate, ch, goals, seed, K, rng_seed=3, all_attempts=True)
            first, later, never = SR.search_counts(want[1], want[4])
            print(f"{case} exact={exact} {gate}: first / later / never = {first}/{later}/{never}")
            assert first >= 1 and never + later >= 1
            set_gate(s, gate)
            for l in (1, 8, 16):
                s.set_option("lanes_per_elite", l)
                for schedule in ("sequential", "parallel"):
                    s.set_option("search_schedule", schedule)
                    what = f"{case} exact={exact} {gate} lanes {l} {schedule}"
                    same(s.search_batch(p, goals, seed, K, rng_seed=3, all_attempts=True), want, what + " (all)")
                    same(s.search_batch(p, goals, seed, K, rng_seed=3), want[:5], what)
            s.set_option("lanes_per_elite", None)
            s.set_option("search_schedule", None)
    finally:
        s.close()


def global_kw(case):
    return dict(case_kw(case), **GT.GLOBAL_KW)


@pytest.mark.parametrize("case", ["panda", "torso_dual_arm"])
def test_gated_global_search_equals_the_gated_loop_over_the_oracle(O, exact_flavour, case):
    n, k = 32, GT.K_GLOBAL
    with O.math_mode("portable"):
        ch, goals, seed, _ = SR.fixture(case, lambda c: O.Oracle(c).fk, n)
        want = GT.oracle_search_global(O, ch, goals, seed, k, global_kw(case), GATE, rng_seed=SR.RNG_SEED, all_attempts=True)
    first, later, never = SR.search_counts(want[1], want[4])
    print(f"{case} [{exact_flavour}] global: first / later / never = {first}/{later}/{never}")
    assert first + later >= 1 and never >= 1 and (want[6] == GT.GATE_REFUSED).any() and (want[6] > 0).any()
    s = pk.Solver(ch, device=0, strict=True)
    try:
        p = pk.default_params(mode=0, **global_kw(case))
        set_gate(s, GATE)
        same(s.search_global_batch(p, goals, seed, k, rng_seed=SR.RNG_SEED, all_attempts=True), want, f"{case} (all)")
        same(s.search_global_batch(p, goals, seed, k, rng_seed=SR.RNG_SEED), want[:5], case)
    finally:
        s.close()


@pytest.mark.parametrize("exact", [None, False], ids=["default_exact", "fast"])
@pytest.mark.parametrize("case", ["panda", "torso_dual_arm"])
def test_gated_global_search_equals_the_gated_loop_over_the_handle(O, case, exact):
    n, k = 32, GT.K_GLOBAL
    s, ch, goals, seed, _ = handle_fixture(case, exact, n)
    try:
        p = pk.default_params(mode=0, **global_kw(case))
        set_gate(s, None)
        want = GT.handle_search_global(s, p, GATE, ch, goals, seed, k, rng_seed=3, all_attempts=True)
        first, later, never = SR.search_counts(want[1], want[4])
        print(f"{case} exact={exact} global: first / later / never = {first}/{later}/{never}")
        assert first + later >= 1 and never >= 1
        set_gate(s, GATE)
        same(s.search_global_batch(p, goals, seed, k, rng_seed=3, all_attempts=True), want, f"{case} exact={exact} (all)")
        same(s.search_global_batch(p, goals, seed, k, rng_seed=3), want[:5], f"{case} exact={exact}")
    finally:
        s.close()


@pytest.mark.parametrize("exact", [None, False], ids=["default_exact", "fast"])
def test_without_a_gate_nothing_changes(O, exact):
    """gate unset, gate set and cleared, gate set on a call without return_approximate_solution: a fresh handle's
    results, in both modes; solve_batch and solve_paths ignore a gate"""
    fresh, ch, goals, seed, p = handle_fixture("panda", exact)
    s = pk.Solver(ch, device=0, exact=exact)
    try:
        pg = pk.default_params(mode=0, **global_kw("panda"))
        exact_mode = dict(case_kw("panda"), return_approximate_solution=0)
        p0 = pk.default_params(mode=1, **exact_mode)
        pg0 = pk.default_params(mode=0, **dict(exact_mode, **GT.GLOBAL_KW))
        n = 32
        want = {"local": fresh.search_batch(p, goals, seed, K, rng_seed=2, all_attempts=True),
                "local, not approximate": fresh.search_batch(p0, goals, seed, 4, rng_seed=2, all_attempts=True),
                "global": fresh.search_global_batch(pg, goals[:n], seed[:n], 2, rng_seed=2, all_attempts=True),
                "global, not approximate": fresh.search_global_batch(pg0, goals[:n], seed[:n], 2, rng_seed=2, all_attempts=True)}
        assert (want["local"][4] == 1).all() and (want["local, not approximate"][4] > 1).any()

        def calls(which):
            got = {}
            if "approximate" in which:
                got["local"] = s.search_batch(p, goals, seed, K, rng_seed=2, all_attempts=True)
                got["global"] = s.search_global_batch(pg, goals[:n], seed[:n], 2, rng_seed=2, all_attempts=True)
            got["local, not approximate"] = s.search_batch(p0, goals, seed, 4, rng_seed=2, all_attempts=True)
            got["global, not approximate"] = s.search_global_batch(pg0, goals[:n], seed[:n], 2, rng_seed=2, all_attempts=True)
            return got

        for state, which in (("no gate yet", "approximate too"), ("gate set", "others"), ("gate cleared", "approximate too")):
            if state == "gate set":
                set_gate(s, GATE)
            if state == "gate cleared":
                set_gate(s, None)
            for name, got in calls(which).items():
                same(got, want[name], f"{state}: {name}")
        set_gate(s, GATE)
        for x, y, w in zip(s.solve_batch(p, goals, seed), fresh.solve_batch(p, goals, seed), SR.NAMES):
            np.testing.assert_array_equal(x, y, err_msg=f"solve_batch ignores the gate: {w}")
        path_goals = goals[:8].reshape(2, 4, 7)
        for x, y in zip(s.solve_paths(p, path_goals, seed[:2]), fresh.solve_paths(p, path_goals, seed[:2])):
            np.testing.assert_array_equal(x, y, err_msg="solve_paths ignores the gate")
    finally:
        s.close()
        fresh.close()


@pytest.mark.parametrize("exact", [None, False], ids=["default_exact", "fast"])
def test_one_gated_attempt_is_solve_batch_and_gate(O, exact):
    s, ch, goals, seed, p = handle_fixture("panda", exact)
    try:
        sol, st, cost, stats = s.solve_batch(p, goals, seed)
        ok = s.gate(p, GT.handle_gate(GATE), goals, seed, sol)
        assert (st > 0).all() and ok.any() and (~ok).any()
        set_gate(s, GATE)
        got = s.search_batch(p, goals, seed, 1)
        np.testing.assert_array_equal(got[1], np.where(ok, st, GT.GATE_REFUSED))
        np.testing.assert_array_equal(got[0], np.where(ok[:, None], sol, seed))
        np.testing.assert_array_equal(got[2], cost)   # the cost and the counters stay what the solve returned:
        np.testing.assert_array_equal(got[3], stats)  # the gate's evaluation is no cost_fn invocation
        assert (got[4] == 1).all()
        pg = pk.default_params(mode=0, **global_kw("panda"))
        sol, st, cost, stats = s.solve_batch(pg, goals, seed, rng_seed=4)
        ok = s.gate(pg, GT.handle_gate(GATE), goals, seed, sol)
        got = s.search_global_batch(pg, goals, seed, 1, rng_seed=4)
        np.testing.assert_array_equal(got[1], np.where(ok & (st > 0), st, np.where(st > 0, GT.GATE_REFUSED, st)))
        np.testing.assert_array_equal(got[0], np.where((ok | ~(st > 0))[:, None], sol, seed))
        np.testing.assert_array_equal(got[2], cost)
        np.testing.assert_array_equal(got[3], stats)
    finally:
        s.close()


@pytest.mark.parametrize("exact", [None, False], ids=["default_exact", "fast"])
def test_gated_shards_with_matching_offsets_equal_one_call(O, exact):
    s, ch, goals, seed, p = handle_fixture("panda_unbounded", exact)
    try:
        set_gate(s, GATE)
        whole = s.search_batch(p, goals, seed, K, rng_seed=5, problem_offset=1000, all_attempts=True)
        lo = s.search_batch(p, goals[:40], seed[:40], K, rng_seed=5, problem_offset=1000, all_attempts=True)
        hi = s.search_batch(p, goals[40:], seed[40:], K, rng_seed=5, problem_offset=1040, all_attempts=True)
        same([np.concatenate([a, b]) for a, b in zip(lo, hi)], whole, "local 40 + 24")
        assert (whole[4] > 1).any() and (whole[1] == GT.GATE_REFUSED).any() and (whole[1] > 0).any()
        pg = pk.default_params(mode=0, **global_kw("panda_unbounded"))
        n, k = 32, GT.K_GLOBAL
        whole = s.search_global_batch(pg, goals[:n], seed[:n], k, rng_seed=5, problem_offset=1000, all_attempts=True)
        lo = s.search_global_batch(pg, goals[:20], seed[:20], k, rng_seed=5, problem_offset=1000, all_attempts=True)
        hi = s.search_global_batch(pg, goals[20:n], seed[20:n], k, rng_seed=5, problem_offset=1020, all_attempts=True)
        same([np.concatenate([a, b]) for a, b in zip(lo, hi)], whole, "global 20 + 12")
        assert (whole[4] > 1).any()
    finally:
        s.close()
