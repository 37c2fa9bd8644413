"""The approximate-solution gate inside the restart searches (CPU, oracle only): the normative gated loops of
tests/gate_reference.py over the CPU oracle on the `panda` fixture must reach EVERY class -- accepted at attempt 0 with
either status, refused by the solution test, refused by the joint limit, accepted at a later attempt, never accepted --
under both oracle math modes, so that the GPU comparison (tests/test_gpu_search_gate.py) cannot pass on one branch
only; what the gate is made of; the declarations."""
import os
import re

import numpy as np
import pytest

from tests import gate_reference as GT
from tests import search_reference as SR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
B = 64


@pytest.fixture(params=["portable", "fma"])
def mode(request):
    return request.param


def classes(O, kw, gate, n=B, k=GT.K):
    """(the six class sizes, the masks of attempt 0, the ungated status of attempt 0, the gated loop's results)"""
    ch, goals, seed, _ = SR.fixture("panda", lambda c: O.Oracle(c).fk, n)
    o = O.Oracle(ch)
    p = O.default_params(mode=1, **kw)
    sol0, st0, _, _ = o.solve_batch(p, goals, seed, num_threads=O.max_threads())
    m = GT.attempt0_classes(GT.oracle_cost(o), p, gate, goals, seed, sol0, st0)
    got = GT.oracle_search(O, ch, goals, seed, k, kw, gate, rng_seed=SR.RNG_SEED)
    st, att = got[1], got[4]
    later, never = (st > 0) & (att > 1), ~(st > 0)
    sizes = tuple(int(x.sum()) for x in m) + (int(later.sum()), int(never.sum()))
    return sizes, m, st0, got, (ch, goals, seed, p, o)


def check_loop_against_attempt0(m, got, k):
    ok1, ok2, by_test, by_joint = m
    sol, st, cost, stats, att = got
    accepted0 = ok1 | ok2
    assert (att[accepted0] == 1).all() and (att[~accepted0] > 1).all()
    assert (st[ok1] == 1).all() and (st[ok2] == 2).all()
    assert set(np.unique(st[~(st > 0)])) == {GT.GATE_REFUSED}  # (approximate mode: the solver itself never fails)
    assert (att[~(st > 0)] == k).all()


def test_panda_fixture_reaches_every_class(oracle_mod, mode):
    O = oracle_mod
    with O.math_mode(mode):
        sizes, m, st0, got, (ch, goals, seed, p, o) = classes(O, GT.PANDA_KW, GT.PANDA_GATE)
    print(f"[{mode}] status 1 / status 2 / refused by the test / by the joint limit / later / never = {sizes}")
    assert all(n >= 1 for n in sizes), sizes
    assert sum(sizes[:4]) == B and sizes[0] + sizes[1] + sizes[4] + sizes[5] == B
    check_loop_against_attempt0(m, got, GT.K)
    # a refused answer is the seed; the cost stays what the solve returned
    refused = ~(got[1] > 0)
    np.testing.assert_array_equal(got[0][refused], seed[refused])
    assert (got[2][refused] > 0).all()
    # without the gate -- none set, or the call not in approximate mode -- the loop is search_reference's
    with O.math_mode(mode):
        plain = SR.oracle_search(O, ch, goals, seed, GT.K, GT.PANDA_KW, rng_seed=SR.RNG_SEED)
        for x, y, w in zip(GT.oracle_search(O, ch, goals, seed, GT.K, GT.PANDA_KW, None, rng_seed=SR.RNG_SEED), plain, SR.NAMES):
            np.testing.assert_array_equal(x, y, err_msg=w)
        kw = dict(GT.PANDA_KW, return_approximate_solution=0)
        for x, y, w in zip(GT.oracle_search(O, ch, goals, seed, 2, kw, GT.PANDA_GATE, rng_seed=SR.RNG_SEED),
                           SR.oracle_search(O, ch, goals, seed, 2, kw, rng_seed=SR.RNG_SEED), SR.NAMES):
            np.testing.assert_array_equal(x, y, err_msg=w)
    assert (plain[4] == 1).all()  # (today: attempt 0 closes every problem)


def test_the_joint_limit_refuses_a_success(oracle_mod, mode):
    """cost_threshold 1e-3: more answers pass the solver's own test, and the joint limit refuses some of THOSE.  The
    class "accepted at attempt 0 with status 2" is empty here by construction, not by luck: status 2 means the answer
    failed the solver's test at 1e-3, the gate applies the same frame tests and the same goals at 6e-4 < 1e-3, so it
    fails the gate too.  The other five classes must be reached."""
    O = oracle_mod
    kw = dict(GT.PANDA_KW, cost_threshold=1e-3)
    with O.math_mode(mode):
        sizes, m, st0, got, _ = classes(O, kw, GT.PANDA_GATE)
    print(f"[{mode}] status 1 / status 2 / refused by the test / by the joint limit / later / never = {sizes}; "
          f"status-1 answers the joint limit refuses: {int((m[3] & (st0 == 1)).sum())}")
    assert sizes[1] == 0 and all(n >= 1 for i, n in enumerate(sizes) if i != 1), sizes
    assert (m[3] & (st0 == 1)).sum() >= 1
    check_loop_against_attempt0(m, got, GT.K)


def test_a_gate_without_thresholds_is_the_frame_tests(oracle_mod, mode):
    O = oracle_mod
    gate = GT.Gate(0.0, 0.0)
    with O.math_mode(mode):
        ch, goals, seed, _ = SR.fixture("panda", lambda c: O.Oracle(c).fk, B)
        o = O.Oracle(ch)
        p = O.default_params(mode=1, **GT.PANDA_KW)
        assert p.position_scale > 0 and p.rotation_scale > 0
        sol, st, _, _ = o.solve_batch(p, goals, seed, num_threads=O.max_threads())
        ok = GT.gate_pass(GT.oracle_cost(o), p, gate, goals, seed, sol)
        frames = np.array([O.frame_test(O.pose12(goals[b]), o.fk_matrix(sol[b]), p.position_threshold, p.orientation_threshold)
                           for b in range(B)])
        # ... whatever the joint goals say: with the weight a thousand times larger the verdict is the same
        heavy = O.default_params(mode=1, **dict(GT.PANDA_KW, minimal_displacement_weight=1.0))
        ok_heavy = GT.gate_pass(GT.oracle_cost(o), heavy, gate, goals, seed, sol)
        with_goals = np.asarray(GT.oracle_cost(o)(heavy, goals, seed, sol)[1]) != 0
    np.testing.assert_array_equal(ok, frames)
    np.testing.assert_array_equal(ok_heavy, frames)
    assert frames.any() and (~frames).any()
    assert (frames & ~with_goals).any()  # (the goal test would have refused some of them)


def test_gate_written_as_the_reference_writes_it():
    """a NaN threshold limits nothing, a NaN difference does not trip the limit, the limit itself is allowed"""
    seed = np.zeros((4, 2))
    q = np.array([[0.0, 2.5], [0.0, np.nextafter(2.5, 3.0)], [np.nan, 0.0], [0.0, -3.0]])
    np.testing.assert_array_equal(GT.joint_test(GT.Gate(0.0, 2.5), seed, q), [True, False, True, False])
    for thr in (0.0, -1.0, float("nan")):
        assert GT.joint_test(GT.Gate(0.0, thr), seed, q).all()


def test_global_mode_reaches_every_group(oracle_mod, mode):
    O = oracle_mod
    kw = dict(GT.PANDA_KW, **GT.GLOBAL_KW)
    with O.math_mode(mode):
        ch, goals, seed, _ = SR.fixture("panda", lambda c: O.Oracle(c).fk, 32)
        got = GT.oracle_search_global(O, ch, goals, seed, GT.K_GLOBAL, kw, GT.PANDA_GATE, rng_seed=SR.RNG_SEED)
    st, att = got[1], got[4]
    first, later, never = SR.search_counts(st, att)
    print(f"[{mode}] global mode: accepted at once / later / never = {first}/{later}/{never}")
    assert first >= 1 and later >= 1 and never >= 1 and first + later + never == 32
    assert (att[~(st > 0)] == GT.K_GLOBAL).all() and set(np.unique(st[~(st > 0)])) == {GT.GATE_REFUSED}
    np.testing.assert_array_equal(got[0][~(st > 0)], seed[~(st > 0)])


def test_header_and_bindings_declare_the_gate():
    header = open(os.path.join(ROOT, "include", "pick_ik_amd.h")).read()
    begin, end = header.index("[host-api-begin]"), header.index("[host-api-end]")
    for name in ("pikamd_gate_batch", "pikamd_set_approximate_gate"):
        m = re.search(r"\b" + name + r"\s*\(", header)
        assert m and begin < m.start() < end, name
    m = re.search(r"#define\s+PIKAMD_GATE_REFUSED\s+\(-1002\)", header)
    assert m and begin < m.start() < end
    assert begin < header.index("typedef struct pikamd_gate") < end
    assert "attempt 0 always closes a problem (attempts == 1 everywhere).  A batch" not in header
    import __graft_entry__ as g
    g.build()
    import pick_ik_amd as pk
    from pick_ik_amd import solver
    assert pk.GATE_REFUSED == GT.GATE_REFUSED == -1002
    assert [f[0] for f in pk.Gate._fields_] == ["cost_threshold", "joint_threshold"]
    for strict in (False, True):
        L = solver.lib(strict)
        for name in ("pikamd_gate_batch", "pikamd_set_approximate_gate"):
            assert name in solver.EXPORTED_SYMBOLS
            assert getattr(L, name).argtypes is not None, name
    for name in ("gate", "set_approximate_gate", "clear_approximate_gate"):
        assert callable(getattr(pk.Solver, name))


def test_gate_kernels_are_reached_from_no_profiled_translation_unit():
    """the gate lives in the search and restart units: pik_inst.hip, whose source hash the committed profiles carry,
    reads none of it, and the constants every kernel reads (ConstsK) do not hold it"""
    from pick_ik_amd import build as Bd
    for f in Bd._deps("pik_inst.hip", True) + Bd._deps("pik_path_inst.hip", True):
        if os.path.basename(f) == "pick_ik_amd.h":  # (declares the host entry points to everyone)
            continue
        text = Bd._strip_comments(open(f).read())
        assert "gate_params" not in text and "GATE_REFUSED" not in text, f
