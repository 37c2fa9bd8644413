"""Cartesian paths from a pose with a memetic start (CPU): the normative loop of pikamd_search_global_paths
(tests/globalpath_reference.py) over the CPU oracle on the fixtures of the GPU tests -- each must reach EVERY class it
claims under both oracle math modes, so that the GPU comparison (tests/test_gpu_globalpath.py) cannot pass on one branch
only --, the loop's own consequences (one waypoint is the global-mode restart search; one attempt is a global solve +
the path loop; shards with matching offsets give the answers of one call; totals is the sum of every row of every
attempt), the declarations, the shape checks and the resource ledger of the new kernels."""
import csv
import os
import re
import subprocess

import numpy as np
import pytest

from tests import globalpath_reference as GP
from tests import path_reference as PR
from tests import search_global_reference as SGR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("pikamd_search_global_paths", "pikamd_search_global_paths_device", "pikamd_search_global_paths_kernel_name")
#: the classes of the fixtures (the order of startpath_reference.CLASSES), counted on the CPU oracle when the feature
#: was specified
SPECIFIED = {("panda", "fma"): (13, 3, 22, 6, 10, 21), ("panda", "portable"): (13, 4, 20, 6, 11, 20),
             ("ur5", "fma"): (11, 3, 26, 9, 8, 21), ("ur5", "portable"): (11, 3, 26, 9, 8, 21),
             ("panda_unbounded", "fma"): (15, 2, 21, 3, 10, 19), ("panda_unbounded", "portable"): (15, 2, 20, 3, 11, 19),
             ("torso_dual_arm", "fma"): (27, 7, 12, 6, 18, 0), ("torso_dual_arm", "portable"): (25, 10, 11, 2, 18, 0)}


@pytest.fixture(params=["portable", "fma"])
def mode(request):
    return request.param


def oracle_fixture(O, case):
    return GP.fixture(case, lambda ch: O.Oracle(ch).fk)


_runs = {}


def oracle_run(O, case, mode):
    """the loop over the oracle on a fixture, once per (case, math mode); nobody changes what it returns"""
    if (case, mode) not in _runs:
        with O.math_mode(mode):
            ch, goals, seed, K, step = oracle_fixture(O, case)
            out = GP.oracle_search_global_paths(O, ch, goals, seed, K, step, kw=GP.params_kw(case), rng_seed=GP.RNG_SEED,
                                                trace=True)
        _runs[(case, mode)] = (ch, goals, seed, K, step, out)
    return _runs[(case, mode)]


@pytest.mark.parametrize("case", list(GP.CASES))
def test_fixture_reaches_every_class_it_claims(oracle_mod, mode, case):
    ch, goals, seed, K, step, out = oracle_run(oracle_mod, case, mode)
    c = GP.counts(out[:7], out[7])
    print(f"{case} [{mode}]: " + ", ".join(f"{n} {k}" for n, k in zip(c, GP.CLASSES)))
    assert all(c[k] >= 1 for k in GP.CASES[case][2]), (case, mode, c)
    assert step is not None or c[5] == 0
    assert c[0] + c[1] + c[2] + c[4] == len(seed)
    assert c == SPECIFIED[(case, mode)]
    sol, st, cost, stats, reached, attempts, totals, tr = out
    W = goals.shape[1]
    assert ((reached == W) | (attempts == K)).all() and (attempts >= 1).all()
    assert (reached[-GP.FAR:] == 0).all()  # (the paths out of reach)
    # the kept rows are a path: held waypoints in front, one stop, not-attempted rows behind it
    for p in range(len(seed)):
        assert (st[p, :reached[p]] > 0).all()
        assert reached[p] == W or st[p, reached[p]] <= 0
        assert (st[p, reached[p] + 1:] == PR.NOT_ATTEMPTED).all()
        np.testing.assert_array_equal(reached[p], tr.reached[p].max())
        assert tr.kept[p] == int(np.argmax(tr.reached[p]))  # (the first among equals)
    # a failed waypoint 0 returns the seed in every row
    never = reached == 0
    np.testing.assert_array_equal(sol[never], np.repeat(seed[never][:, None], W, axis=1))


def test_one_waypoint_is_the_global_restart_search(oracle_mod, mode):
    O = oracle_mod
    with O.math_mode(mode):
        ch, goals, seed, K, _ = oracle_fixture(O, "panda")
        kw = GP.params_kw("panda")
        one, local = GP.oracle_callables(O, ch, kw)
        got = GP.reference_search_global_paths(one, local, ch, goals[:, :1], seed, K, np.full(ch.dof, 1e-6),
                                               rng_seed=GP.RNG_SEED)
        want = SGR.reference_search(one, ch, goals[:, 0], seed, K, rng_seed=GP.RNG_SEED)
        first = [one(goals[b:b + 1, 0], seed[b:b + 1], seed[b:b + 1], SGR.attempt_seed(GP.RNG_SEED, 0), b)[2][0]
                 for b in range(len(seed))]
    solved = want[1] > 0
    assert (solved & (want[4] == 1)).any() and (solved & (want[4] > 1)).any() and (~solved).any()
    np.testing.assert_array_equal(got[0][:, 0], want[0])
    np.testing.assert_array_equal(got[1][:, 0], want[1])
    # (a problem no attempt solved keeps the row of its FIRST attempt -- the first among equals -- where the restart
    #  search reports its last: the cost of such a problem is that of the first attempt's solve)
    np.testing.assert_array_equal(got[2][solved, 0], want[2][solved])
    np.testing.assert_array_equal(got[2][~solved, 0], np.array(first)[~solved])
    np.testing.assert_array_equal(got[4], solved.astype(np.int32))
    np.testing.assert_array_equal(got[5], want[4])
    np.testing.assert_array_equal(got[6], want[3])  # (the search sums its attempts: totals)
    # (no joint-step test at waypoint 0: the tiny limit above refused nothing)
    assert not (got[1] == PR.PATH_JUMP).any()


def test_one_attempt_is_a_global_solve_and_the_path_loop(oracle_mod, mode):
    O = oracle_mod
    with O.math_mode(mode):
        ch, goals, seed, _, step = oracle_fixture(O, "panda")
        one, local = GP.oracle_callables(O, ch, GP.params_kw("panda"))
        got = GP.reference_search_global_paths(one, local, ch, goals, seed, 1, step, rng_seed=GP.RNG_SEED)
        rows = [one(goals[b:b + 1, 0], seed[b:b + 1], seed[b:b + 1], GP.RNG_SEED, b) for b in range(len(seed))]
        sol0, st0, c0, stats0 = (np.concatenate([r[k] for r in rows]) for k in range(4))
        ok = st0 > 0
        rest = PR.reference_paths(local, goals[ok, 1:], sol0[ok], step)
    assert ok.any() and not ok.all() and (got[5] == 1).all()
    np.testing.assert_array_equal(got[0][:, 0], sol0)
    np.testing.assert_array_equal(got[1][:, 0], st0)
    np.testing.assert_array_equal(got[2][:, 0], c0)
    np.testing.assert_array_equal(got[3][:, 0], stats0)
    for k in range(4):
        np.testing.assert_array_equal(got[k][ok, 1:], rest[k], err_msg=GP.NAMES[k])
    np.testing.assert_array_equal(got[4][ok], 1 + rest[4])
    assert (got[4][~ok] == 0).all() and (got[1][~ok, 1:] == PR.NOT_ATTEMPTED).all()
    np.testing.assert_array_equal(got[0][~ok], np.repeat(seed[~ok][:, None], goals.shape[1], axis=1))


def test_half_batches_with_offsets_equal_the_whole(oracle_mod, mode):
    O = oracle_mod
    with O.math_mode(mode):
        ch, goals, seed, K, step = oracle_fixture(O, "panda_unbounded")
        kw = dict(kw=GP.params_kw("panda_unbounded"), rng_seed=5)
        whole = GP.oracle_search_global_paths(O, ch, goals, seed, K, step, **kw)
        lo = GP.oracle_search_global_paths(O, ch, goals[:20], seed[:20], K, step, problem_offset=0, **kw)
        hi = GP.oracle_search_global_paths(O, ch, goals[20:], seed[20:], K, step, problem_offset=20, **kw)
        other = GP.oracle_search_global_paths(O, ch, goals[20:], seed[20:], K, step, problem_offset=0, **kw)
    for w, a, b, name in zip(whole, lo, hi, GP.NAMES):
        np.testing.assert_array_equal(w, np.concatenate([a, b]), err_msg=name)
    assert not np.array_equal(other[0], hi[0])  # (the offset keys the memetic streams and the restarts)


def test_totals_is_the_sum_of_every_row_of_every_attempt(oracle_mod, mode):
    ch, goals, seed, K, step, out = oracle_run(oracle_mod, "panda", mode)
    totals, tr = out[6], out[7]
    want = np.zeros(len(seed), dtype=GP.STATS_DTYPE)
    for idx, rows in tr.attempt_stats:
        for f in GP.STATS_DTYPE.names:
            np.add.at(want[f], idx, rows[f].sum(axis=1))
    np.testing.assert_array_equal(totals, want)
    several = out[5] > 1
    assert several.any() and (totals["cost_evals"][several] > out[3]["cost_evals"][several].sum(axis=1)).all()


def test_header_and_bindings_declare_the_entry_points():
    header = open(os.path.join(ROOT, "include", "pick_ik_amd.h")).read()
    begin, end = header.index("[host-api-begin]"), header.index("[host-api-end]")
    for name in SYMBOLS:
        m = re.search(r"\b" + name + r"\s*\(", header)
        assert m and begin < m.start() < end, name
    text = " ".join(header[header.index("memetic start, Cartesian path behind"):end].replace(" *", " ").split())
    for said in ("p->mode must be 0", "pikamd_search_paths serves it", "the first among equals wins",
                 "one global-mode pikamd_solve_batch followed by one pikamd_solve_paths with p_local",
                 "W = 1 is pikamd_search_global_batch without a gate", "keeps the row of its FIRST attempt",
                 "matching problem_offset", "only a refused jump", "wipeouts, pool_erasures and reserved included",
                 "the approximate-solution gate; all_* rows per attempt; a relative (mean-step) jump threshold; a "
                 "parallel schedule over the attempts", "No completion counters"):
        assert said in text, said
    mirror = open(os.path.join(ROOT, "pick_ik_amd", "host", "pick_ik_amd.hpp")).read()
    assert "ik_memetic_search_paths(" in mirror and "pikamd_search_global_paths(" in mirror
    import __graft_entry__ as g
    g.build()
    import pick_ik_amd as pk
    from pick_ik_amd import solver
    for strict in (False, True):
        L = solver.lib(strict)
        for name in SYMBOLS:
            assert name in solver.EXPORTED_SYMBOLS
            assert getattr(L, name).argtypes is not None, name
    for name in ("search_global_paths", "search_global_paths_device", "search_global_paths_kernel_name"):
        assert callable(getattr(pk.Solver, name))


def test_shape_checks_come_before_the_library():
    """(no GPU here: a call that reached the library would fail for another reason)"""
    import __graft_entry__ as g
    g.build()
    import pick_ik_amd as pk
    s = pk.Solver.__new__(pk.Solver)  # a handle-less object: the checks must raise before anything is called
    s.dof, s.n_tips, s._env_options = 7, 1, lambda: None
    p = pk.default_params()
    goals, seed = np.zeros((4, 3, 7)), np.zeros((4, 7))
    with pytest.raises(ValueError, match="goals"):
        s.search_global_paths(p, np.zeros((4, 7)), seed, 4)
    with pytest.raises(ValueError, match="goals"):
        s.search_global_paths(p, np.zeros((4, 3, 6)), seed, 4)
    with pytest.raises(ValueError, match="at least one waypoint"):
        s.search_global_paths(p, np.zeros((4, 0, 7)), seed, 4)
    with pytest.raises(ValueError, match="seed"):
        s.search_global_paths(p, goals, np.zeros((3, 7)), 4)
    with pytest.raises(ValueError, match="initial_guess"):
        s.search_global_paths(p, goals, seed, 4, initial_guess=np.zeros((4, 6)))
    with pytest.raises(ValueError, match="max_joint_step"):
        s.search_global_paths(p, goals, seed, 4, max_joint_step=np.zeros(6))
    for k in (0, 65):
        with pytest.raises(ValueError, match="max_attempts"):
            s.search_global_paths(p, goals, seed, k)
    with pytest.raises(ValueError, match="W >= 1"):
        s.search_global_paths_device(p, 4, 0, 1, 1, 4, 1, 1)
    s._h = None


def kernel_names(fl, d):
    names = [f"ik_globalpath_prepare_kernel<{d}>", f"ik_globalpath_kernel<{d},false>", f"ik_globalpath_kernel<{d},true>"]
    return names + ([f"ik_globalpath_wide_kernel<{d},{l},{m}>" for l in (16, 8) for m in ("false", "true")] if fl == "fast"
                    else [f"ik_globalpath_team_kernel<{d},{l}>" for l in (16, 4)])


FLAVOURS = (("fast", "pik"), ("exact", "pik_exact"), ("strict", "pik_strict"))
#: what the ledger tests of the other families count kernels by
OTHERS = ("ik_startpath", "::ik_path", "::ik_search", "restart_fold_kernel", "restart_prepare_kernel", "memetic_kernel<",
          "::search_finalize", "route_kernel")


def test_the_family_is_declared_in_the_build_tables_only():
    from pick_ik_amd import build as Bd
    assert Bd.FAMILIES["pik_globalpath_inst.hip"] == (("fast", "exact"), ("strict",))
    assert "pik_globalpath_inst.hip" in Bd.APPENDED_FAMILIES
    assert len(Bd.FLAVOURS) == 5
    for strict, flavours in ((False, ("fast", "exact")), (True, ("strict",))):
        assert not [o for o in Bd.library_objects(strict) if "pik_globalpath" in o[0]]
        objs = [o for o in Bd.link_objects(strict) if "pik_globalpath" in o[0]]
        assert objs == [o for fl in flavours for o in Bd.family_objects("pik_globalpath_inst.hip", fl)]
        assert Bd.link_objects(strict)[:len(Bd.library_objects(strict))] == Bd.library_objects(strict)
        assert Bd.link_objects(strict)[-len(objs):] == objs


def test_ledger_has_the_kernels_for_fast_exact_strict_only():
    import __graft_entry__ as g
    g.build()
    from pick_ik_amd import build as Bd
    rows = Bd.ledger_rows()
    if rows is None:
        pytest.skip("no compiler remarks beside the objects (libraries built elsewhere)")
    have = {(fl, k) for fl, k, _ in rows}
    for fl, ns in FLAVOURS:
        for d in range(1, 17):
            for k in kernel_names(fl, d):
                assert (fl, f"{ns}::{k}") in have, (fl, k)
    assert not [k for fl, k in have if fl in ("common", "common_goals") and "globalpath" in k]


def test_committed_ledger_has_the_kernels():
    path = os.path.join(ROOT, "profiles", "r06_kernel_resources.csv")
    rows = {(r["flavour"], r["kernel"]): r for r in csv.DictReader(open(path))}
    n = [k for k in rows if "::ik_globalpath" in k[1]]
    assert len(n) == 16 * (7 + 5 + 5)
    assert {fl for fl, _ in n} == {"fast", "exact", "strict"}
    for fl, ns in FLAVOURS:
        for d in range(1, 17):
            for k in kernel_names(fl, d):
                assert (fl, f"{ns}::{k}") in rows, (fl, k)
    # no name is counted by the tests of the other families
    for _, k in n:
        for other in OTHERS:
            assert other not in k, (k, other)
    # a fast tail kernel spills no vector register where its ik_path_* twin of the same length does not
    for fl, k in n:
        if fl == "fast" and "prepare" not in k:
            twin = rows[(fl, k.replace("ik_globalpath", "ik_path"))]
            assert int(rows[(fl, k)]["vgpr_spills"]) <= int(twin["vgpr_spills"]), (k, rows[(fl, k)]["vgpr_spills"])


def test_the_kernels_are_reached_from_no_existing_translation_unit():
    from pick_ik_amd import build as Bd
    for tu in ("pik_inst.hip", "pik_path_inst.hip", "pik_search_inst.hip", "pik_startpath_inst.hip", "pik_route_inst.hip",
               "pik_restart_inst.hip"):
        for f in Bd._deps(tu, True):
            assert "pik_globalpath" not in os.path.basename(f), (tu, f)
    # (the C ABI translation unit reads the host side only: no device code there)
    ops = Bd._strip_comments(open(os.path.join(Bd.CSRC, "pik_globalpath_ops.hpp")).read())
    assert not re.search(r"__global__|__device__|__shared__|__constant__", ops)
    assert not any(os.path.basename(f) == "pik_globalpath.hpp" for f in Bd._deps("pik_amd.hip", True))
    assert any(os.path.basename(f) == "pik_globalpath_ops.hpp" for f in Bd._deps("pik_amd.hip", True))


def test_a_hip_caller_compiles_against_the_header_and_the_mirror(tmp_path):
    """tests/native/globalpath_api_check.hip calls the three entry points and Solver::ik_memetic_search_paths from a
    .hip file: hipcc compiles it for gfx950, device pass included"""
    from pick_ik_amd import build as Bd
    src = os.path.join(ROOT, "tests", "native", "globalpath_api_check.hip")
    r = subprocess.run([Bd.hipcc(), "--offload-arch=gfx950", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-c", src, "-o",
                        str(tmp_path / "globalpath_api_check.o")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
