"""Memetic IK with random restarts (CPU): the normative loop of pikamd_search_global_batch
(tests/search_global_reference.py) over the CPU oracle on the fixtures of the global-mode search tests -- each must
reach EVERY class (solved at the first attempt, at a later one, never) under both oracle math modes, so that the GPU
comparison (tests/test_gpu_search_global.py) cannot pass on one branch only --, the loop's own consequences, the
attempt seeds, the declarations, the binding's argument checks and the resource ledger of the new kernels."""
import os
import re

import numpy as np
import pytest

from tests import search_global_reference as GR
from tests import search_reference as SR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("pikamd_search_global_batch", "pikamd_search_global_batch_device")
B, K = 64, GR.K


@pytest.fixture(params=["portable", "fma"])
def mode(request):
    return request.param


def oracle_fixture(O, case, n=B):
    return GR.fixture(case, lambda ch: O.Oracle(ch).fk, n)


def classes(O, case, kw):
    ch, goals, seed = oracle_fixture(O, case)
    sol, st, cost, stats, att = GR.oracle_search(O, ch, goals, seed, K, kw, rng_seed=GR.RNG_SEED)
    assert (att[st <= 0] == K).all() and (att >= 1).all() and (att <= K).all()
    return SR.search_counts(st, att)


@pytest.mark.parametrize("case", list(GR.GENERATIONS))
def test_fixture_reaches_every_class(oracle_mod, mode, case):
    O = oracle_mod
    with O.math_mode(mode):
        first, later, never = classes(O, case, GR.params_kw(case))
    print(f"{case} [{mode}]: first / later / never = {first}/{later}/{never}")
    assert first >= 1 and later >= 1 and never >= 1
    assert first + later + never == B


@pytest.mark.parametrize("name,more", [("species", dict(memetic_num_threads=2)),
                                       ("elite_1", dict(memetic_elite_size=1, memetic_population_size=9))])
def test_panda_variations_reach_every_class(oracle_mod, mode, name, more):
    O = oracle_mod
    with O.math_mode(mode):
        first, later, never = classes(O, "panda", GR.params_kw("panda", **more))
    print(f"panda {name} [{mode}]: first / later / never = {first}/{later}/{never}")
    assert first >= 1 and later >= 1 and never >= 1


def test_approximate_mode_closes_every_problem_at_attempt_0(oracle_mod, mode):
    O = oracle_mod
    with O.math_mode(mode):
        ch, goals, seed = oracle_fixture(O, "panda")
        got = GR.oracle_search(O, ch, goals, seed, K, GR.params_kw("panda", return_approximate_solution=1))
    assert (got[4] == 1).all() and (got[1] > 0).all()


def test_attempt_0_is_a_plain_solve_batch(oracle_mod, mode):
    """one attempt from a valid start: the caller's seed unchanged, problem_offset + b -- solve_batch on the batch"""
    O = oracle_mod
    with O.math_mode(mode):
        ch, goals, seed = oracle_fixture(O, "panda")
        kw = GR.params_kw("panda")
        got = GR.oracle_search(O, ch, goals, seed, 1, kw, rng_seed=7, problem_offset=100)
        want = O.Oracle(ch).solve_batch(O.default_params(mode=0, **kw), goals, seed, rng_seed=7, problem_offset=100,
                                        num_threads=O.max_threads())
        every = GR.oracle_search(O, ch, goals[:8], seed[:8], K, kw, rng_seed=7, problem_offset=100, all_attempts=True)
    for x, y, w in zip(got[:4], want, SR.NAMES):
        np.testing.assert_array_equal(x, y, err_msg=w)
    assert (got[4] == 1).all()
    np.testing.assert_array_equal(every[5][:, 0], want[0][:8])
    np.testing.assert_array_equal(every[6][:, 0], want[1][:8])


def test_attempt_seeds():
    assert GR.attempt_seed(5, 0) == 5
    assert GR.attempt_seed(5, 1) == (1 << 32) + 5
    assert GR.attempt_seed((1 << 32) + 5, 3) == (4 << 32) + 5
    assert GR.attempt_seed((0xffffffff << 32) + 5, 1) == 5  # wraps mod 2^64
    assert GR.attempt_seed((0xffffffff << 32) + 5, 2) == (1 << 32) + 5
    # the low word, which the stream id is folded into, is the caller's in every attempt
    assert {GR.attempt_seed(0x1234, a) & 0xffffffff for a in range(64)} == {0x1234}


def test_attempts_draw_from_streams_of_their_own(oracle_mod):
    """the same start under rng_seed_0 and rng_seed_1 is two different searches; the restart states are keyed by the
    caller's seed alone"""
    O = oracle_mod
    with O.math_mode("fma"):
        ch, goals, seed = oracle_fixture(O, "panda", 8)
        one = GR.oracle_solve_one(O, ch, O.default_params(mode=0, **GR.params_kw("panda")))
        r0 = one(goals[:1], seed[:1], seed[:1], GR.attempt_seed(1, 0), 0)
        r1 = one(goals[:1], seed[:1], seed[:1], GR.attempt_seed(1, 1), 0)
    assert not np.array_equal(r0[0], r1[0]) or r0[3]["cost_evals"][0] != r1[3]["cost_evals"][0]
    t = SR.starts(ch, seed, K, rng_seed=1)
    np.testing.assert_array_equal(t[0, 1], SR.draw(ch, 1, 0, 1, t[0, 0]))


def test_header_and_bindings_declare_the_entry_points():
    header = open(os.path.join(ROOT, "include", "pick_ik_amd.h")).read()
    begin, end = header.index("[host-api-begin]"), header.index("[host-api-end]")
    for name in SYMBOLS:
        m = re.search(r"\b" + name + r"\s*\(", header)
        assert m and begin < m.start() < end, name
    import __graft_entry__ as g
    g.build()
    import pick_ik_amd as pk
    from pick_ik_amd import solver
    for strict in (False, True):
        L = solver.lib(strict)
        for name in SYMBOLS:
            assert name in solver.EXPORTED_SYMBOLS
            assert getattr(L, name).argtypes is not None, name
    for name in ("search_global_batch", "search_global_batch_device"):
        assert callable(getattr(pk.Solver, name))
    mirror = open(os.path.join(ROOT, "pick_ik_amd", "host", "pick_ik_amd.hpp")).read()
    assert "ik_memetic_search_batch" in mirror and "pikamd_search_global_batch(" in mirror


def test_shape_checks_come_before_the_library():
    """(no GPU here: a call that reached the library would fail for another reason)"""
    import __graft_entry__ as g
    g.build()
    import pick_ik_amd as pk
    s = pk.Solver.__new__(pk.Solver)  # a handle-less object: the checks must raise before anything is called
    s.dof, s.n_tips, s._env_options = 7, 1, lambda: None
    p = pk.default_params(mode=0)
    with pytest.raises(ValueError, match="goal_pos_quat"):
        s.search_global_batch(p, np.zeros((4, 6)), np.zeros((4, 7)), 4)
    with pytest.raises(ValueError, match="seed"):
        s.search_global_batch(p, np.zeros((4, 7)), np.zeros((3, 7)), 4)
    with pytest.raises(ValueError, match="initial_guess"):
        s.search_global_batch(p, np.zeros((4, 7)), np.zeros((4, 7)), 4, initial_guess=np.zeros((4, 6)))
    for k in (0, 65):
        with pytest.raises(ValueError, match="max_attempts"):
            s.search_global_batch(p, np.zeros((4, 7)), np.zeros((4, 7)), k)
    s._h = None


def test_restart_launcher_leaves_the_existing_translation_units_alone():
    from pick_ik_amd import build as Bd
    for src in ("pik_inst.hip", "pik_path_inst.hip", "pik_search_inst.hip", "pik_route_inst.hip"):
        for f in Bd._deps(src, True):
            assert "pik_restart" not in os.path.basename(f), (src, f)
    objs = [o for strict in (False, True) for o in Bd.library_objects(strict) if "pik_restart" in o[0]]
    assert objs == [o for fl in Bd.ROUTE_FLAVOURS + ("strict",) for o in Bd.family_objects("pik_restart_inst.hip", fl)]
    assert len(objs) == 16 * 5 and {o[1] for o in objs} == {"pik_restart_inst.hip"}


def test_restart_scratch_is_launch_solves_layout():
    """The restart launcher sizes the slot's solver scratch itself, in front of attempt 0, so that no attempt grows it
    under kernels in flight, and it is the layout launch_solve and the routed launcher use by construction: every term
    of the layout is written in ONE file under csrc/, the plan header, and in none of the three launcher headers; the
    record rows of a chain length (StateRows<D>, device side) are handed to it in one place, which all three call."""
    from pick_ik_amd import build as Bd

    text = {f: Bd._strip_comments(open(os.path.join(Bd.CSRC, f)).read()) for f in sorted(os.listdir(Bd.CSRC))}
    launchers = ("pik_launch.hpp", "pik_route.hpp", "pik_restart.hpp")
    terms = ("(size_t)B * (size_t)S", "sizeof(double) * d_rows * recs", "sizeof(long long) * l_rows * recs",
             "sizeof(int) * i_rows * recs", "s->chain.bounded_mask != ((1u << s->chain.dof) - 1u)",
             "(size_t)population * (1 + D) + ((size_t)population + 1) / 2", "(off_cnt + 64 + 63) / 64 * 64",
             # the two survivor lists and the stored population
             "sizeof(int) * 2 * (size_t)B", "sizeof(double) * 2 * pop_stride * (size_t)B * (size_t)S")
    for t in terms:
        assert [f for f in text if t in text[f]] == ["pik_memetic_plan.hpp"], t
    for name in ("off_d", "off_l", "off_i", "off_list", "off_pop", "pop_stride"):
        assigned = re.compile(r"(?<![.\w])" + name + r" = ")  # (the launchers read the fields, none computes one)
        assert assigned.search(text["pik_memetic_plan.hpp"]), name
        assert not [f for f in launchers if assigned.search(text[f])], name
    # the rows of a record: named once, in the function that makes the layout for a chain length ...
    for rows in ("(size_t)StateRows<D>::D_ROWS(pk.elites)", "StateRows<D>::L_ROWS", "StateRows<D>::I_ROWS"):
        assert [(f, text[f].count(rows)) for f in launchers if rows in text[f]] == [("pik_launch.hpp", 1)], rows
    make = text["pik_launch.hpp"]
    make = make[make.index("MemeticScratch memetic_scratch("):make.index("struct MemeticCall")]
    assert all(rows in make for rows in ("D_ROWS(pk.elites)", "L_ROWS", "I_ROWS", "chain_has_unbounded(s)"))
    # ... which the three launchers call (launch_solve and the routed one through MemeticCall::scratch), and nothing
    # else makes one
    assert text["pik_launch.hpp"].count("memetic_scratch<D>(") == 1 and "m.scratch(pk, B)" in text["pik_launch.hpp"]
    assert "m.scratch(pk, B)" in text["pik_route.hpp"] and "memetic_scratch" not in text["pik_route.hpp"]
    assert text["pik_restart.hpp"].count("memetic_scratch<D>(s, pk, B, S)") == 1 and "m.scratch(pk, B)" in text["pik_restart.hpp"]
    assert [f for f in text if "MemeticScratch(" in text[f]] == ["pik_launch.hpp", "pik_memetic_plan.hpp"]
    assert text["pik_launch.hpp"].count("MemeticScratch(") == 1


def test_committed_ledger_has_the_restart_kernels_without_scratch_or_spill():
    import csv
    path = os.path.join(ROOT, "profiles", "r06_kernel_resources.csv")
    rows = {(r["flavour"], r["kernel"]): r for r in csv.DictReader(open(path))}
    n = [k for k in rows if "::restart_prepare_kernel" in k[1] or "::restart_fold_kernel" in k[1]]
    assert len(n) == 16 * 5 * 2
    assert {fl for fl, _ in n} == {"fast", "exact", "strict", "common", "common_goals"}
    for k in n:
        r = rows[k]
        assert int(r["vgpr_spills"]) == 0 and int(r["sgpr_spills"]) == 0 and int(r["scratch_bytes_per_lane"]) == 0, k
