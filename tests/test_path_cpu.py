"""Waypoint paths (CPU): the normative loop of pikamd_solve_paths (tests/path_reference.py) over the CPU oracle on the
fixtures of the path tests -- they must exercise EVERY branch (complete paths, paths stopped inside, paths stopped at
waypoint 0, refused jumps), so that the GPU comparison (tests/test_gpu_path.py) cannot pass on one branch only --,
the shape of the rows behind a stop, the declarations, the resource ledger of the new kernels, and the device source
of the existing kernels, which this feature must leave alone."""
import os
import re

import numpy as np
import pytest

from pick_ik_amd import robots
from tests import path_reference as PR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# pick_ik_amd/build.py flavour_sha of the five kernel namespaces: the DEVICE source pik_inst.hip is compiled from --
# every file of csrc/ and include/ it reads except the host-only launcher headers (build.HOST_LAUNCH_HEADERS) and the
# public header's host API block.  The text is the one of the commit BEFORE the path kernels (they, and every kernel
# family since, live in translation units of their own, and nothing the existing kernels are compiled from may change
# with them); the values were re-recorded, on that unchanged text, when flavour_sha stopped reading the launcher
# headers (before: 932c715cd5f4522d, d4b4bcfc18f1f403, b5498b8fb01f4fb9, 131a72a184826437, d5356aa7eb0fef00).
# profiles/roofline_inputs.json stores the hashes of the text its counters were taken on, which are older than either
# set: bench.py reports roofline.inputs_stale for them.
PARENT_FLAVOUR_SHA = {
    "pik": "70ff2d32d099c466",
    "pik_common": "6fcc4560a2f0128b",
    "pik_common_goals": "dcb1de80a0c1b540",
    "pik_exact": "95c3ffff63c7bf7c",
    "pik_strict": "b40303f3db0f66f7",
}


def oracle_paths(O, chain, goals, start, max_joint_step=None, **kw):
    o = O.Oracle(chain)
    p = O.default_params(mode=1, **kw)
    return PR.reference_paths(lambda g, s: o.solve_batch(p, g, s, num_threads=O.max_threads()), goals, start,
                              max_joint_step)


@pytest.fixture(params=["portable", "fma"])
def mode(request):
    return request.param


def test_panda_straight_lines_cover_every_branch(oracle_mod, mode):
    O = oracle_mod
    ch = robots.panda()
    with O.math_mode(mode):
        goals, start = PR.straight_lines(ch, O.Oracle(ch).fk)
        sol, st, cost, stats, reached = oracle_paths(O, ch, goals, start)
        _, stj, _, _, _ = oracle_paths(O, ch, goals, start, max_joint_step=np.full(ch.dof, 0.1))
    complete, inside, at0, _ = PR.path_counts(st)
    print(f"panda straight lines [{mode}]: complete {complete}, stopped inside {inside}, at waypoint 0 {at0}; with the "
          f"0.1 step limit: jump stops {PR.path_counts(stj)[3]}")
    assert complete >= 16 and inside >= 8 and at0 >= 4
    assert PR.path_counts(stj)[3] >= 1
    assert complete + inside + at0 == goals.shape[0]


def test_torso_dual_arm_joint_lines_cover_both_branches(oracle_mod, mode):
    O = oracle_mod
    ch = robots.torso_dual_arm()
    with O.math_mode(mode):
        goals, start = PR.joint_lines(ch, O.Oracle(ch).fk)
        _, st, _, _, _ = oracle_paths(O, ch, goals, start)
    complete, inside, at0, _ = PR.path_counts(st)
    print(f"torso_dual_arm joint-space lines [{mode}]: complete {complete}, stopped inside {inside}, at waypoint 0 {at0}")
    assert goals.shape == (32, 16, 2, 7)
    assert complete >= 16 and inside >= 1


def test_every_gpu_case_has_complete_and_stopped_paths(oracle_mod, mode):
    """the cases tests/test_gpu_path.py compares with the oracle: each must reach both branches, in both math modes"""
    from tests.test_gpu_path import ORACLE_CASES, assert_both_branches, oracle_case
    O = oracle_mod
    for case in ORACLE_CASES:
        with O.math_mode(mode):
            want = oracle_case(O, case)[5]
        print(f"{case} [{mode}]: complete / inside / at 0 / jumps = {PR.path_counts(want[1])}")
        assert_both_branches(want[1], f"{case} [{mode}]")
    with O.math_mode(mode):
        assert PR.path_counts(oracle_case(O, "floating_panda")[5][1])[3] >= 1  # (its stops are refused jumps)


def test_a_hip_caller_compiles_against_the_header_and_the_mirror(tmp_path):
    """tests/native/path_api_check.hip calls the three entry points and Solver::ik_gradient_paths from a .hip file:
    hipcc compiles it for gfx950, device pass included (where host function bodies are checked too)"""
    import subprocess
    from pick_ik_amd import build as B
    src = os.path.join(ROOT, "tests", "native", "path_api_check.hip")
    r = subprocess.run([B.hipcc(), "--offload-arch=gfx950", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-c", src, "-o",
                        str(tmp_path / "path_api_check.o")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    # ... and every declaration of the public header is seen by the device pass (nothing hidden from it)
    header = open(os.path.join(ROOT, "include", "pick_ik_amd.h")).read()
    assert "__HIP_DEVICE_COMPILE__" not in header and "__HIPCC__" not in header


def test_rows_behind_a_stop_and_reached(oracle_mod, mode):
    O = oracle_mod
    ch = robots.panda()
    with O.math_mode(mode):
        goals, start = PR.straight_lines(ch, O.Oracle(ch).fk)
        sol, st, cost, stats, reached = oracle_paths(O, ch, goals, start, max_joint_step=np.full(ch.dof, 0.1))
    P, W = st.shape
    seen_behind = 0
    for p in range(P):
        held = st[p] > 0
        n = int(np.argmin(held)) if not held.all() else W  # leading held waypoints
        assert reached[p] == n
        assert set(st[p, :n]) <= {1, 2}
        if n == W:
            continue
        # the waypoint the path stopped at: what the call returned, the last held configuration as its solution
        last = sol[p, n - 1] if n > 0 else start[p]
        assert st[p, n] in (-31, PR.PATH_JUMP)
        np.testing.assert_array_equal(sol[p, n], last)
        assert stats["cost_evals"][p, n] > 0
        # ... and everything behind it: not attempted
        np.testing.assert_array_equal(sol[p, n + 1:], np.broadcast_to(last, (W - n - 1, ch.dof)))
        assert (st[p, n + 1:] == PR.NOT_ATTEMPTED).all() and (cost[p, n + 1:] == 0.0).all()
        for f in stats.dtype.names:
            assert (stats[f][p, n + 1:] == 0).all()
        seen_behind += W - n - 1
    assert seen_behind > 0
    # a held waypoint moved no variable further than the limit
    prev = np.concatenate([start[:, None, :], sol[:, :-1, :]], axis=1)
    assert (np.abs(sol - prev)[st > 0] <= 0.1).all()


def test_step_limit_entries_at_or_below_zero_set_no_limit(oracle_mod):
    O = oracle_mod
    ch = robots.panda()
    with O.math_mode("fma"):
        goals, start = PR.straight_lines(ch, O.Oracle(ch).fk, P=16, W=8)
        a = oracle_paths(O, ch, goals, start)
        b = oracle_paths(O, ch, goals, start, max_joint_step=np.array([0.0, -1.0, 0.0, np.nan, 0.0, -0.1, 0.0]))
    for x, y in zip(a, b):
        np.testing.assert_array_equal(x, y)


def test_header_and_bindings_declare_the_path_entry_points():
    header = open(os.path.join(ROOT, "include", "pick_ik_amd.h")).read()
    for name in ("pikamd_solve_paths", "pikamd_solve_paths_device", "pikamd_path_kernel_name"):
        assert re.search(r"\b" + name + r"\s*\(", header), name
    assert re.search(r"#define\s+PIKAMD_NOT_ATTEMPTED\s+0\b", header)
    assert re.search(r"#define\s+PIKAMD_PATH_JUMP\s+\(-1001\)", header)
    import __graft_entry__ as g
    g.build()
    import pick_ik_amd as pk
    from pick_ik_amd import solver
    assert (pk.NOT_ATTEMPTED, pk.PATH_JUMP) == (0, -1001) == (PR.NOT_ATTEMPTED, PR.PATH_JUMP)
    for strict in (False, True):
        L = solver.lib(strict)
        for name in ("pikamd_solve_paths", "pikamd_solve_paths_device", "pikamd_path_kernel_name"):
            assert name in solver.EXPORTED_SYMBOLS
            assert getattr(L, name).argtypes is not None, name
    for name in ("solve_paths", "solve_paths_device", "path_kernel_name"):
        assert callable(getattr(pk.Solver, name))


def test_shape_checks_come_before_the_library():
    """(no GPU here: a call that reached the library would fail for another reason)"""
    import __graft_entry__ as g
    g.build()
    import pick_ik_amd as pk
    s = pk.Solver.__new__(pk.Solver)  # a handle-less object: the checks must raise before anything is called
    s.dof, s.n_tips, s._env_options = 7, 1, lambda: None
    p = pk.default_params(mode=1)
    with pytest.raises(ValueError, match="goals"):
        s.solve_paths(p, np.zeros((4, 8, 6)), np.zeros((4, 7)))
    with pytest.raises(ValueError, match="goals"):
        s.solve_paths(p, np.zeros((4, 7)), np.zeros((4, 7)))
    with pytest.raises(ValueError, match="waypoint"):
        s.solve_paths(p, np.zeros((4, 0, 7)), np.zeros((4, 7)))
    with pytest.raises(ValueError, match="start"):
        s.solve_paths(p, np.zeros((4, 8, 7)), np.zeros((3, 7)))
    with pytest.raises(ValueError, match="max_joint_step"):
        s.solve_paths(p, np.zeros((4, 8, 7)), np.zeros((4, 7)), max_joint_step=np.zeros(6))
    s.n_tips = 2
    with pytest.raises(ValueError, match="goals"):
        s.solve_paths(p, np.zeros((4, 8, 7)), np.zeros((4, 7)))
    s._h = None


def test_ledger_has_path_kernels_for_fast_exact_strict_only():
    import __graft_entry__ as g
    g.build()
    from pick_ik_amd import build as B
    rows = B.ledger_rows()
    if rows is None:
        pytest.skip("no compiler remarks beside the objects (libraries built elsewhere)")
    have = {(fl, k) for fl, k, _ in rows}
    for fl, ns in (("fast", "pik"), ("exact", "pik_exact"), ("strict", "pik_strict")):
        for d in range(1, 17):
            assert (fl, f"{ns}::ik_path_kernel<{d},false>") in have, (fl, d)
            assert (fl, f"{ns}::ik_path_kernel<{d},true>") in have, (fl, d)
            wide = [f"ik_path_wide_kernel<{d},{l},{m}>" for l in (16, 8) for m in ("false", "true")] if fl == "fast" \
                else [f"ik_path_team_kernel<{d},{l}>" for l in (16, 4)]
            for k in wide:
                assert (fl, f"{ns}::{k}") in have, (fl, k)
    assert not [k for fl, k in have if fl in ("common", "common_goals") and "ik_path" in k]


def test_committed_ledger_has_the_path_kernels():
    import csv
    rows = {(r["flavour"], r["kernel"]): r for r in csv.DictReader(open(os.path.join(ROOT, "profiles", "r06_kernel_resources.csv")))}
    n = [k for k in rows if "::ik_path" in k[1]]
    assert len(n) == 16 * (6 + 4 + 4)
    assert {fl for fl, _ in n} == {"fast", "exact", "strict"}
    # the fast flavour's path kernels inline everything: no stack, no spilled vector register (the exact flavours' call
    # their evaluations and carry a stack, as their ik_gradient kernels do; the growth gate of
    # tests/test_kernel_resources_cpu.py holds them to the committed figures)
    for k in n:
        if k[0] == "fast":
            assert int(rows[k]["vgpr_spills"]) == 0 and int(rows[k]["scratch_bytes_per_lane"]) == 0, k


def test_existing_kernels_are_compiled_from_untouched_text():
    from pick_ik_amd import build as B
    assert set(B.FLAVOUR_FLAGS) == set(PARENT_FLAVOUR_SHA)
    assert {ns: B.flavour_sha(ns) for ns in B.FLAVOUR_FLAGS} == PARENT_FLAVOUR_SHA
    # ... and the path kernels are reached from none of it
    for f in B._deps("pik_inst.hip", True):
        assert "pik_path" not in os.path.basename(f)
