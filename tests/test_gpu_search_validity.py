"""The validity step of the restart searches on the GPU: with a sphere model on the handle (pikamd_set_validity_model)
pikamd_search_batch and pikamd_search_global_batch test every answer of status > 0 where the reference calls the
solution callback (src/pick_ik_plugin.cpp:269-274), behind the approximate-solution gate, and restart on a refusal.

Everything compares at tolerance zero, in every output array, with tests/validity_reference.py: the loop over the CPU
oracle for the exact builds, the loop over the handle's own solve + gate + validity -- the definition -- for every
flavour.  The fixture is the Panda of search_reference (B = 64, rng_seed 1) with robots.panda_spheres(); local mode
runs K = 8 attempts, global mode gate_reference.GLOBAL_KW with 4.  tests/test_validity_cpu.py shows that the oracle
loops meet the fixture conditions; they are asserted here again on what the GPU returns."""
import numpy as np
import pytest

import pick_ik_amd as pk
from pick_ik_amd import robots
from pick_ik_amd.solver import STATS_DTYPE
from tests import gate_reference as GT
from tests import search_reference as SR
from tests import validity_reference as V
from tests.hip_buffers import DeviceBuffers

pytestmark = pytest.mark.gpu
ALL_NAMES = SR.NAMES + ("all_solution", "all_status")
B = 64
GATE = GT.PANDA_GATE
FAMILIES = {"local": (1, GT.K, dict(GT.PANDA_KW)), "global": (0, GT.K_GLOBAL, dict(GT.PANDA_KW, **GT.GLOBAL_KW))}
NO_PAIRS = np.zeros((0, 2), dtype=np.int32)


@pytest.fixture(scope="module")
def O(oracle_mod):
    import __graft_entry__ as g
    g.build()
    return oracle_mod


def same(a, b, what=""):
    assert len(a) == len(b), what
    for x, y, w in zip(a, b, ALL_NAMES):
        np.testing.assert_array_equal(x, y, err_msg=f"{what}: {w}")


def set_gate(s, gate):
    if gate is None:
        s.clear_approximate_gate()
    else:
        s.set_approximate_gate(gate.cost_threshold, gate.joint_threshold)


def search(s, family, p, goals, seed, K, **kw):
    return (s.search_batch if family == "local" else s.search_global_batch)(p, goals, seed, K, **kw)


_oracle_cache = {}


def oracle_reference(O, flavour, family, gated):
    """(chain, goals, seed, the loop without the model, the loop with it), every attempt recorded -- computed once per
    exact build, family and gate, and left unchanged"""
    key = (flavour, family, gated)
    if key not in _oracle_cache:
        _, K, kw = FAMILIES[family]
        with O.math_mode("portable"):
            ch, goals, seed, _ = SR.fixture("panda", lambda c: O.Oracle(c).fk, B)
            loop = V.oracle_search if family == "local" else V.oracle_search_global
            gate = GATE if gated else None
            plain = loop(O, ch, goals, seed, K, kw, gate, None, rng_seed=SR.RNG_SEED, all_attempts=True)
            want = loop(O, ch, goals, seed, K, kw, gate, robots.panda_spheres(), rng_seed=SR.RNG_SEED, all_attempts=True)
        for a in plain + want:
            a.setflags(write=False)
        _oracle_cache[key] = (ch, goals, seed, plain, want)
    return _oracle_cache[key]


def fixture_conditions(plain, got, gated, what):
    refused0, valid0, rescued, ended = V.fixture_counts(plain[6], got[6], got[1], got[4])
    both = int(((plain[6] > 0) & (got[6] == V.VALIDITY_REFUSED)).sum())
    print(f"{what}: refused at attempt 0 / valid at attempt 0 / rescued / ending refused = {refused0}/{valid0}/{rescued}/{ended}; "
          f"rows the gate passes and the test refuses: {both}")
    assert refused0 >= 8 and valid0 >= 8 and rescued >= 2 and ended >= 1, (what, refused0, valid0, rescued, ended)
    assert not gated or both >= 1, what


@pytest.mark.parametrize("gated", [False, True], ids=["no_gate", "gate"])
def test_local_search_equals_the_loop_over_the_oracle(O, exact_flavour, gated):
    """both schedules x 1 / 4 / 16 lanes per unit, with and without all_*"""
    ch, goals, seed, plain, want = oracle_reference(O, exact_flavour, "local", gated)
    mode, K, kw = FAMILIES["local"]
    s = pk.Solver(ch, device=0, strict=True)
    try:
        p = pk.default_params(mode=mode, **kw)
        set_gate(s, GATE if gated else None)
        same(s.search_batch(p, goals, seed, K, rng_seed=SR.RNG_SEED, all_attempts=True), plain, "no model yet")
        s.set_validity_model(*robots.panda_spheres())
        names = set()
        for lanes in (1, 4, 16):
            s.set_option("lanes_per_elite", lanes)
            for schedule in ("sequential", "parallel"):
                s.set_option("search_schedule", schedule)
                names.add(s.search_kernel_name(p, B, K))
                what = f"local [{exact_flavour}] gate {gated} lanes {lanes} {schedule}"
                got = s.search_batch(p, goals, seed, K, rng_seed=SR.RNG_SEED, all_attempts=True)
                same(got, want, what + " (all)")
                same(s.search_batch(p, goals, seed, K, rng_seed=SR.RNG_SEED), want[:5], what)
        fixture_conditions(plain, got, gated, f"local [{exact_flavour}] gate {gated}")
        assert {k for _, k in names} == {1, K} and len({n for n, _ in names}) == 3, names
    finally:
        s.close()


@pytest.mark.parametrize("gated", [False, True], ids=["no_gate", "gate"])
def test_global_search_equals_the_loop_over_the_oracle(O, exact_flavour, gated):
    ch, goals, seed, plain, want = oracle_reference(O, exact_flavour, "global", gated)
    mode, K, kw = FAMILIES["global"]
    s = pk.Solver(ch, device=0, strict=True)
    try:
        p = pk.default_params(mode=mode, **kw)
        set_gate(s, GATE if gated else None)
        s.set_validity_model(*robots.panda_spheres())
        got = s.search_global_batch(p, goals, seed, K, rng_seed=SR.RNG_SEED, all_attempts=True)
        same(got, want, f"global [{exact_flavour}] gate {gated} (all)")
        same(s.search_global_batch(p, goals, seed, K, rng_seed=SR.RNG_SEED), want[:5], f"global [{exact_flavour}] gate {gated}")
        fixture_conditions(plain, got, gated, f"global [{exact_flavour}] gate {gated}")
    finally:
        s.close()


def handle_fixture(exact):
    s = pk.Solver(robots.panda(), device=0, exact=exact)
    ch, goals, seed, _ = SR.fixture("panda", lambda _: s.fk, B)
    return s, ch, goals, seed


@pytest.mark.parametrize("gated", [False, True], ids=["no_gate", "gate"])
@pytest.mark.parametrize("family", ["local", "global"])
def test_search_equals_the_loop_over_the_handle(O, family, gated):
    """the definition: solve + gate + Solver.validity on the same handle, attempt by attempt"""
    s, ch, goals, seed = handle_fixture(None)
    try:
        mode, K, kw = FAMILIES[family]
        p = pk.default_params(mode=mode, **kw)
        gate = GATE if gated else None
        s.set_validity_model(*robots.panda_spheres())
        loop = V.handle_search if family == "local" else V.handle_search_global
        want = loop(s, p, gate, ch, goals, seed, K, rng_seed=SR.RNG_SEED, all_attempts=True)
        assert (want[6] == V.VALIDITY_REFUSED).any() and (want[1] > 0).any()
        set_gate(s, gate)
        same(search(s, family, p, goals, seed, K, rng_seed=SR.RNG_SEED, all_attempts=True), want, f"{family} gate {gated} (all)")
        same(search(s, family, p, goals, seed, K, rng_seed=SR.RNG_SEED), want[:5], f"{family} gate {gated}")
    finally:
        s.close()


@pytest.mark.parametrize("case", ["rr", "ur5"])
def test_other_chain_lengths_equal_the_loop_over_the_handle(O, case):
    """two and six joints (other instantiations of the step than the Panda's seven), both families, no gate"""
    s = pk.Solver(SR.CASES[case][0](), device=0)
    try:
        ch, goals, seed, kw = SR.fixture(case, lambda _: s.fk, 32)
        last = ch.dof - 1
        # the last link, a link frame's origin in front of it, and an obstacle around the first target, 0.6 of the
        # targets' median distance from their mean wide: some targets are inside it, most are not
        pos = goals[:, :3]
        radius = 0.6 * float(np.median(np.linalg.norm(pos - pos.mean(axis=0), axis=1)))
        spheres = [(last, (0.0, 0.0, 0.05), 0.1), (last // 2, (0.0, 0.0, 0.0), 0.05), (-1, tuple(pos[0]), radius)]
        s.set_validity_model(spheres, [[0, 2], [0, 1]])
        for family, K, more in (("local", 4, {}), ("global", 2, GT.GLOBAL_KW)):
            p = pk.default_params(mode=1 if family == "local" else 0, **dict(kw, **more))
            loop = V.handle_search if family == "local" else V.handle_search_global
            want = loop(s, p, None, ch, goals, seed, K, rng_seed=SR.RNG_SEED, all_attempts=True)
            print(f"{case} {family}: rows refused {(want[6] == V.VALIDITY_REFUSED).sum()}, solved {(want[6] > 0).sum()}")
            assert (want[6] == V.VALIDITY_REFUSED).any() and (want[6] > 0).any()
            same(search(s, family, p, goals, seed, K, rng_seed=SR.RNG_SEED, all_attempts=True), want, f"{case} {family}")
    finally:
        s.close()


def test_fast_handle_local_search_is_refused_and_global_search_is_served(O):
    s, ch, goals, seed = handle_fixture(False)
    try:
        _, K, kw = FAMILIES["local"]
        p = pk.default_params(mode=1, **kw)
        before = s.search_batch(p, goals, seed, K, rng_seed=SR.RNG_SEED)
        s.set_validity_model(*robots.panda_spheres())
        with pytest.raises(pk.PickIkAmdError, match="error -4.*arithmetic"):
            s.search_batch(p, goals, seed, K, rng_seed=SR.RNG_SEED)
        _, Kg, kwg = FAMILIES["global"]
        pg = pk.default_params(mode=0, **kwg)
        assert s.kernel_name(pg).startswith("pik")  and not s.kernel_name(pg).startswith("pik_exact")
        for gate in (None, GATE):
            set_gate(s, None)
            want = V.handle_search_global(s, pg, gate, ch, goals, seed, Kg, rng_seed=SR.RNG_SEED, all_attempts=True)
            assert (want[6] == V.VALIDITY_REFUSED).any() and (want[1] > 0).any()
            set_gate(s, gate)
            same(s.search_global_batch(pg, goals, seed, Kg, rng_seed=SR.RNG_SEED, all_attempts=True), want, f"fast, gate {gate}")
        s.clear_validity_model()
        set_gate(s, None)
        same(s.search_batch(p, goals, seed, K, rng_seed=SR.RNG_SEED), before, "model cleared: served again")
    finally:
        s.close()


@pytest.mark.parametrize("exact", [None, False], ids=["default_exact", "fast"])
def test_without_a_model_nothing_changes(O, exact):
    """no model, a model without pairs, a model set and cleared: the arrays of a handle that never had one, in both
    families; solve_batch, solve_paths and search_paths ignore a model"""
    fresh, ch, goals, seed = handle_fixture(exact)
    s = pk.Solver(ch, device=0, exact=exact)
    try:
        pl = pk.default_params(mode=1, **FAMILIES["local"][2])
        pg = pk.default_params(mode=0, **FAMILIES["global"][2])
        n = 32
        want = {"local": fresh.search_batch(pl, goals, seed, GT.K, rng_seed=2, all_attempts=True),
                "global": fresh.search_global_batch(pg, goals[:n], seed[:n], 2, rng_seed=2, all_attempts=True)}

        def calls(local):
            got = {"global": s.search_global_batch(pg, goals[:n], seed[:n], 2, rng_seed=2, all_attempts=True)}
            if local:
                got["local"] = s.search_batch(pl, goals, seed, GT.K, rng_seed=2, all_attempts=True)
            return got

        spheres, pairs = robots.panda_spheres()
        for state in ("no model yet", "no pairs", "set and cleared"):
            if state == "no pairs":
                s.set_validity_model(spheres, NO_PAIRS)
            if state == "set and cleared":
                s.set_validity_model(spheres, pairs)
                s.clear_validity_model()
            # (a fast handle's local search is refused while a model is set, even one without pairs)
            for name, got in calls(local=exact is None or state != "no pairs").items():
                same(got, want[name], f"{state}: {name}")
        s.set_validity_model(spheres, pairs)
        for x, y, w in zip(s.solve_batch(pl, goals, seed), fresh.solve_batch(pl, goals, seed), SR.NAMES):
            np.testing.assert_array_equal(x, y, err_msg=f"solve_batch ignores the model: {w}")
        for x, y, w in zip(s.solve_batch(pg, goals[:n], seed[:n], rng_seed=3), fresh.solve_batch(pg, goals[:n], seed[:n], rng_seed=3),
                           SR.NAMES):
            np.testing.assert_array_equal(x, y, err_msg=f"solve_batch (global mode) ignores the model: {w}")
        path_goals = goals[:8].reshape(2, 4, 7)
        for x, y in zip(s.solve_paths(pl, path_goals, seed[:2]), fresh.solve_paths(pl, path_goals, seed[:2])):
            np.testing.assert_array_equal(x, y, err_msg="solve_paths ignores the model")
        for x, y in zip(s.search_paths(pl, path_goals, seed[:2], 3, rng_seed=2), fresh.search_paths(pl, path_goals, seed[:2], 3, rng_seed=2)):
            np.testing.assert_array_equal(x, y, err_msg="search_paths ignores the model")
    finally:
        s.close()
        fresh.close()


def test_one_attempt_is_solve_gate_and_validity(O):
    """max_attempts = 1: pikamd_solve_batch + pikamd_gate_batch + pikamd_validity_batch; the cost and the counters stay
    what the solve returned"""
    s, ch, goals, seed = handle_fixture(None)
    try:
        s.set_validity_model(*robots.panda_spheres())
        set_gate(s, GATE)
        for family in ("local", "global"):
            mode, _, kw = FAMILIES[family]
            p = pk.default_params(mode=mode, **kw)
            sol, st, cost, stats = s.solve_batch(p, goals, seed, rng_seed=4)
            passed = s.gate(p, GT.handle_gate(GATE), goals, seed, sol)
            ok = s.validity(sol)[0]
            status = np.where(st > 0, np.where(passed, np.where(ok, st, V.VALIDITY_REFUSED), GT.GATE_REFUSED), st)
            assert (status == V.VALIDITY_REFUSED).any() and (status == GT.GATE_REFUSED).any() and (status > 0).any()
            got = search(s, family, p, goals, seed, 1, rng_seed=4)
            np.testing.assert_array_equal(got[1], status, err_msg=family)
            np.testing.assert_array_equal(got[0], np.where((status > 0)[:, None] | (st <= 0)[:, None], sol, seed), err_msg=family)
            np.testing.assert_array_equal(got[2], cost, err_msg=family)
            np.testing.assert_array_equal(got[3], stats, err_msg=family)
            assert (got[4] == 1).all()
    finally:
        s.close()


def test_shards_with_matching_offsets_equal_one_call(O):
    s, ch, goals, seed = handle_fixture(None)
    try:
        s.set_validity_model(*robots.panda_spheres())
        set_gate(s, GATE)
        for family, cut in (("local", 40), ("global", 24)):
            mode, K, kw = FAMILIES[family]
            p = pk.default_params(mode=mode, **kw)
            whole = search(s, family, p, goals, seed, K, rng_seed=5, problem_offset=1000, all_attempts=True)
            lo = search(s, family, p, goals[:cut], seed[:cut], K, rng_seed=5, problem_offset=1000, all_attempts=True)
            hi = search(s, family, p, goals[cut:], seed[cut:], K, rng_seed=5, problem_offset=1000 + cut, all_attempts=True)
            same([np.concatenate([a, b]) for a, b in zip(lo, hi)], whole, f"{family} {cut} + {B - cut}")
            assert (whole[6] == V.VALIDITY_REFUSED).any() and (whole[4] > 1).any()
    finally:
        s.close()


@pytest.mark.parametrize("exact", [None, False], ids=["default_exact", "fast"])
def test_device_entry_points_equal_the_host_ones(O, exact):
    s, ch, goals, seed = handle_fixture(exact)
    d = None
    try:
        s.set_validity_model(*robots.panda_spheres())
        set_gate(s, GATE)
        d = DeviceBuffers()
        dg, ds = d.upload(goals), d.upload(seed)
        for family in ("local", "global") if exact is None else ("global",):
            mode, K, kw = FAMILIES[family]
            p = pk.default_params(mode=mode, **kw)
            want = search(s, family, p, goals, seed, K, rng_seed=SR.RNG_SEED, all_attempts=True)
            assert (want[6] == V.VALIDITY_REFUSED).any()
            out = dict(sol=d.alloc(8 * 7 * B), st=d.alloc(4 * B), cost=d.alloc(8 * B), stats=d.alloc(STATS_DTYPE.itemsize * B),
                       att=d.alloc(4 * B), all_sol=d.alloc(8 * 7 * B * K), all_st=d.alloc(4 * B * K))
            enqueue = s.search_batch_device if family == "local" else s.search_global_batch_device
            enqueue(p, B, dg, ds, K, out["sol"], out["st"], d_cost=out["cost"], d_stats=out["stats"], d_attempts=out["att"],
                    d_all_solution=out["all_sol"], d_all_status=out["all_st"], rng_seed=SR.RNG_SEED, slot=3)
            d.sync()
            got = (d.download(out["sol"], (B, 7), np.float64), d.download(out["st"], B, np.int32),
                   d.download(out["cost"], B, np.float64), d.download(out["stats"], B, STATS_DTYPE),
                   d.download(out["att"], B, np.int32), d.download(out["all_sol"], (B, K, 7), np.float64),
                   d.download(out["all_st"], (B, K), np.int32))
            same(got, want, f"{family} exact={exact}: device entry point")
    finally:
        if d is not None:
            d.free()
        s.close()
