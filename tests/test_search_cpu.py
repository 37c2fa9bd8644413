"""Local IK with random restarts (CPU): the normative loop of pikamd_search_batch (tests/search_reference.py) over the
CPU oracle on the fixtures of the search tests -- each must reach EVERY class (solved at the first attempt, solved at a
later one, never solved) under both oracle math modes, so that the GPU comparison (tests/test_gpu_search.py) cannot
pass on one branch only --, the loop's own consequences (one attempt is solve_batch; shards with matching offsets give
the answers of one call), the restart draw, the declarations and the resource ledger of the new kernels."""
import os
import re

import numpy as np
import pytest

from tests import search_reference as SR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("pikamd_search_batch", "pikamd_search_batch_device", "pikamd_search_kernel_name")
B, K = 64, 4


@pytest.fixture(params=["portable", "fma"])
def mode(request):
    return request.param


def oracle_fixture(O, case, n=B):
    return SR.fixture(case, lambda ch: O.Oracle(ch).fk, n)


@pytest.mark.parametrize("case", list(SR.CASES))
def test_fixture_reaches_every_class(oracle_mod, mode, case):
    O = oracle_mod
    with O.math_mode(mode):
        ch, goals, seed, kw = oracle_fixture(O, case)
        sol, st, cost, stats, att = SR.oracle_search(O, ch, goals, seed, K, kw, rng_seed=SR.RNG_SEED)
    first, later, never = SR.search_counts(st, att)
    print(f"{case} [{mode}]: first / later / never = {first}/{later}/{never}")
    assert first >= 1 and later >= 1 and never >= 1
    assert first + later + never == B
    assert (att[st <= 0] == K).all() and (att >= 1).all() and (att <= K).all()


def test_one_attempt_is_solve_batch(oracle_mod, mode):
    O = oracle_mod
    with O.math_mode(mode):
        ch, goals, seed, kw = oracle_fixture(O, "panda")
        got = SR.oracle_search(O, ch, goals, seed, 1, kw)
        want = O.Oracle(ch).solve_batch(O.default_params(mode=1), goals, seed, num_threads=O.max_threads())
    for x, y, w in zip(got[:4], want, SR.NAMES):
        np.testing.assert_array_equal(x, y, err_msg=w)
    assert (got[4] == 1).all()


def test_half_batches_with_offsets_equal_the_whole(oracle_mod, mode):
    O = oracle_mod
    with O.math_mode(mode):
        ch, goals, seed, kw = oracle_fixture(O, "panda_unbounded")
        whole = SR.oracle_search(O, ch, goals, seed, K, kw, rng_seed=5)
        lo = SR.oracle_search(O, ch, goals[:40], seed[:40], K, kw, rng_seed=5, problem_offset=0)
        hi = SR.oracle_search(O, ch, goals[40:], seed[40:], K, kw, rng_seed=5, problem_offset=40)
        other = SR.oracle_search(O, ch, goals[40:], seed[40:], K, kw, rng_seed=5, problem_offset=0)
    for w, a, b, name in zip(whole, lo, hi, SR.NAMES):
        np.testing.assert_array_equal(w, np.concatenate([a, b]), err_msg=name)
    assert not np.array_equal(other[0], hi[0])  # (the offset is what keys the restarts)


def test_all_attempts_rows_are_single_solves_and_leave_the_loop_alone(oracle_mod):
    O = oracle_mod
    with O.math_mode("fma"):
        ch, goals, seed, kw = oracle_fixture(O, "panda", 16)
        plain = SR.oracle_search(O, ch, goals, seed, K, kw)
        every = SR.oracle_search(O, ch, goals, seed, K, kw, all_attempts=True)
    for x, y, w in zip(plain, every[:5], SR.NAMES):
        np.testing.assert_array_equal(x, y, err_msg=w)
    all_sol, all_st = every[5], every[6]
    win = every[4] - 1
    np.testing.assert_array_equal(all_st[np.arange(16), win], every[1])
    np.testing.assert_array_equal(all_sol[np.arange(16), win], every[0])
    assert (all_st[:, 0] > 0).any() and (all_st[win < K - 1][:, -1] != 0).all()  # rows behind a winner are real results


def test_restart_draw(oracle_mod):
    """bounded variables land inside their limits and do not depend on the previous start; unbounded ones within pi
    of it; an invalid or NaN initial guess is re-drawn at epoch 0"""
    ch = SR.panda_unbounded()
    home = np.asarray(SR.robots.PANDA_HOME)
    t = SR.starts(ch, np.stack([home, home + 1.0]), 6, rng_seed=3)
    bounded = np.asarray(ch.bounded, dtype=bool)
    np.testing.assert_array_equal(t[0, 0], home)
    assert (t[:, 1:, bounded] >= ch.qmin[bounded]).all() and (t[:, 1:, bounded] <= ch.qmax[bounded]).all()
    assert (np.abs(np.diff(t[:, :, ~bounded], axis=1)) <= np.pi).all()
    assert len({tuple(x) for x in t.reshape(-1, ch.dof)}) >= 11  # the states differ by problem and attempt
    same_b = SR.starts(ch, np.stack([home, home]), 3, rng_seed=3)
    np.testing.assert_array_equal(same_b[0], t[0, :3])
    assert SR.valid(ch, home) and not SR.valid(ch, np.where(np.arange(7) == 3, np.nan, home))
    far = home.copy()
    far[0] = 1.0e3  # (unbounded: no limit to be outside of)
    assert SR.valid(ch, far)
    bad = home.copy()
    bad[1] = ch.qmax[1] + 0.5
    s = SR.starts(ch, home[None], 2, rng_seed=3, initial_guess=bad[None])
    np.testing.assert_array_equal(s[0, 0], SR.draw(ch, 3, 0, 0, bad))
    np.testing.assert_array_equal(s[0, 1], SR.draw(ch, 3, 0, 1, s[0, 0]))


def test_header_and_bindings_declare_the_search_entry_points():
    header = open(os.path.join(ROOT, "include", "pick_ik_amd.h")).read()
    begin, end = header.index("[host-api-begin]"), header.index("[host-api-end]")
    for name in SYMBOLS:
        m = re.search(r"\b" + name + r"\s*\(", header)
        assert m and begin < m.start() < end, name
    m = re.search(r"#define\s+PIKAMD_MAX_ATTEMPTS\s+64\b", header)
    assert m and begin < m.start() < end
    import __graft_entry__ as g
    g.build()
    import pick_ik_amd as pk
    from pick_ik_amd import solver
    assert pk.MAX_ATTEMPTS == SR.MAX_ATTEMPTS == 64
    for strict in (False, True):
        L = solver.lib(strict)
        for name in SYMBOLS:
            assert name in solver.EXPORTED_SYMBOLS
            assert getattr(L, name).argtypes is not None, name
    for name in ("search_batch", "search_batch_device", "search_kernel_name"):
        assert callable(getattr(pk.Solver, name))


def test_shape_checks_come_before_the_library():
    """(no GPU here: a call that reached the library would fail for another reason)"""
    import __graft_entry__ as g
    g.build()
    import pick_ik_amd as pk
    s = pk.Solver.__new__(pk.Solver)  # a handle-less object: the checks must raise before anything is called
    s.dof, s.n_tips, s._env_options = 7, 1, lambda: None
    p = pk.default_params(mode=1)
    with pytest.raises(ValueError, match="goal_pos_quat"):
        s.search_batch(p, np.zeros((4, 6)), np.zeros((4, 7)), 4)
    with pytest.raises(ValueError, match="seed"):
        s.search_batch(p, np.zeros((4, 7)), np.zeros((3, 7)), 4)
    with pytest.raises(ValueError, match="initial_guess"):
        s.search_batch(p, np.zeros((4, 7)), np.zeros((4, 7)), 4, initial_guess=np.zeros((4, 6)))
    for k in (0, 65):
        with pytest.raises(ValueError, match="max_attempts"):
            s.search_batch(p, np.zeros((4, 7)), np.zeros((4, 7)), k)
    s._h = None


def test_ledger_has_search_kernels_for_fast_exact_strict_only():
    import __graft_entry__ as g
    g.build()
    from pick_ik_amd import build as Bd
    rows = Bd.ledger_rows()
    if rows is None:
        pytest.skip("no compiler remarks beside the objects (libraries built elsewhere)")
    have = {(fl, k) for fl, k, _ in rows}
    for fl, ns in (("fast", "pik"), ("exact", "pik_exact"), ("strict", "pik_strict")):
        for d in range(1, 17):
            names = [f"ik_search_kernel<{d},false>", f"ik_search_kernel<{d},true>", f"search_finalize_kernel<{d}>"]
            names += [f"ik_search_wide_kernel<{d},{l},{m}>" for l in (16, 8) for m in ("false", "true")] if fl == "fast" \
                else [f"ik_search_team_kernel<{d},{l}>" for l in (16, 4)]
            for k in names:
                assert (fl, f"{ns}::{k}") in have, (fl, k)
    assert not [k for fl, k in have if fl in ("common", "common_goals") and "search" in k]


def test_committed_ledger_has_the_search_kernels():
    import csv
    path = os.path.join(ROOT, "profiles", "r06_kernel_resources.csv")
    rows = {(r["flavour"], r["kernel"]): r for r in csv.DictReader(open(path))}
    n = [k for k in rows if "::ik_search" in k[1] or "::search_finalize" in k[1]]
    assert len(n) == 16 * (7 + 5 + 5)
    assert {fl for fl, _ in n} == {"fast", "exact", "strict"}
    for k in n:  # the fast flavour's search kernels inline everything: no spilled vector register
        if k[0] == "fast":
            assert int(rows[k]["vgpr_spills"]) == 0, k


def test_search_kernels_are_reached_from_no_existing_translation_unit():
    from pick_ik_amd import build as Bd
    for f in Bd._deps("pik_inst.hip", True) + Bd._deps("pik_path_inst.hip", True):
        assert "pik_search" not in os.path.basename(f)
