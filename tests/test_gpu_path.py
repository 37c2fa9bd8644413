"""Cartesian waypoint paths on the GPU (pikamd_solve_paths): chained local IK in one launch.

Its result is DEFINED as what the loop of local-mode solve_batch calls returns (include/pick_ik_amd.h;
tests/path_reference.py holds that loop), so everything here compares at tolerance zero: against the loop over the CPU
oracle for the exact builds, against the loop over the handle's own solve_batch for the fast flavour, every kernel
variant against every other.  tests/test_path_cpu.py shows that the fixtures reach every branch of the loop."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import pick_ik_amd as pk
from pick_ik_amd import robots
from tests import abi_calls as A
from tests import path_reference as PR
from tests.test_mimic_cpu import CASES, with_mimic

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("solution", "status", "cost", "stats", "reached")


@pytest.fixture(scope="module")
def O(oracle_mod):
    import __graft_entry__ as g
    g.build()
    return oracle_mod


def same(a, b, what=""):
    for x, y, w in zip(a, b, NAMES):
        np.testing.assert_array_equal(x, y, err_msg=f"{what}: {w}")


def mimic_panda():
    name, k, master, mult, off = CASES[0]
    return with_mimic(np.random.default_rng(5 + k), robots.by_name(name), k, master, mult, off)[0]


FLOATING_BASE = (np.arange(7), robots.FLOATING_PANDA_HOME[:7])  # floating_panda: only the arm variables move
# name -> (chain, fixture, solver parameters, step limit).  Every case has complete paths AND stopped ones, under both
# oracle math modes (asserted here and, without a GPU, by tests/test_path_cpu.py): the joint-space lines of
# floating_panda are all solved (its fourteen variables share steps of at most 0.012), so that case runs with a step
# limit of 0.01, which refuses a few of them; the straight lines of the mimic chain stop at once, it takes
# joint-space lines.
ORACLE_CASES = {
    "panda": (robots.panda, "straight", {}, None),
    "panda_displacement": (robots.panda, "straight", dict(minimal_displacement_weight=0.001), None),
    "panda_step_limit": (robots.panda, "straight", {}, 0.1),
    "panda_displacement_step_limit": (robots.panda, "straight", dict(minimal_displacement_weight=0.001), 0.1),
    "ur5": (robots.ur5, "straight", {}, None),
    "panda_on_torso": (robots.panda_on_torso, "straight", {}, None),
    "torso_dual_arm": (robots.torso_dual_arm, "joint", {}, None),
    "floating_panda": (robots.floating_panda, "joint_fixed_base", {}, 0.01),
    "panda_mimic": (mimic_panda, "joint", {}, None),
}


def fixture_of(kind, chain, fk):
    if kind == "straight":
        return PR.straight_lines(chain, fk)
    return PR.joint_lines(chain, fk, fixed=FLOATING_BASE if kind == "joint_fixed_base" else None)


def oracle_case(O, case):
    """(chain, goals, start, step limit, solver parameters, the loop over the oracle) of one case, in the math mode set"""
    make, kind, kw, limit = ORACLE_CASES[case]
    ch = make()
    o = O.Oracle(ch)
    step = None if limit is None else np.full(ch.dof, limit)
    goals, start = fixture_of(kind, ch, o.fk)
    po = O.default_params(mode=1, **kw)
    want = PR.reference_paths(lambda g, sd: o.solve_batch(po, g, sd, num_threads=O.max_threads()), goals, start, step)
    return ch, goals, start, step, kw, want


def assert_both_branches(status, what=""):
    """a case must hold some paths to the end and stop others (a comparison on one branch only shows half)"""
    complete, inside, at0, jumps = PR.path_counts(status)
    assert complete >= 1 and inside + at0 >= 1, (what, complete, inside, at0, jumps)


@pytest.mark.parametrize("case", list(ORACLE_CASES))
def test_paths_equal_the_loop_over_the_oracle(O, exact_flavour, case):
    with O.math_mode("portable"):
        ch, goals, start, step, kw, want = oracle_case(O, case)
    assert_both_branches(want[1], f"{case} [{exact_flavour}]")
    s = pk.Solver(ch, device=0, strict=True)
    try:
        got = s.solve_paths(pk.default_params(mode=1, **kw), goals, start, step)
        print(f"{case} [{exact_flavour}] {s.path_kernel_name(pk.default_params(mode=1, **kw), len(start))}: "
              f"complete / inside / at 0 / jumps = {PR.path_counts(want[1])}")
        same(got, want, f"{case} [{exact_flavour}]")
    finally:
        s.close()


@pytest.mark.parametrize("exact", [None, False], ids=["default_exact", "fast"])
@pytest.mark.parametrize("robot", ["panda", "torso_dual_arm"])
def test_paths_equal_the_loop_over_the_handles_own_solve_batch(O, robot, exact):
    ch = robots.by_name(robot)
    s = pk.Solver(ch, device=0, exact=exact)
    try:
        goals, start = (PR.straight_lines(ch, s.fk) if robot == "panda" else PR.joint_lines(ch, s.fk))
        for kw, limit in (({}, None), (dict(minimal_displacement_weight=0.001), 0.1)):
            p = pk.default_params(mode=1, **kw)
            step = None if limit is None else np.full(ch.dof, limit)
            want = PR.reference_paths(lambda g, sd: s.solve_batch(p, g, sd), goals, start, step)
            got = s.solve_paths(p, goals, start, step)
            same(got, want, f"{robot} exact={exact} {kw} limit {limit}")
            complete, inside, at0, _ = PR.path_counts(want[1])
            assert complete >= 1 and inside + at0 >= 1, (robot, exact, kw, complete, inside, at0)
    finally:
        s.close()


@pytest.mark.parametrize("exact,robot,lanes", [
    (None, "panda", {1: "pik_exact::ik_path_kernel<7,false>", 4: "pik_exact::ik_path_team_kernel<7,4>",
                     16: "pik_exact::ik_path_team_kernel<7,16>"}),
    (False, "panda", {1: "pik::ik_path_kernel<7,false>", 8: "pik::ik_path_wide_kernel<7,8,false>",
                      16: "pik::ik_path_wide_kernel<7,16,false>"}),
    (False, "torso_dual_arm", {1: "pik::ik_path_kernel<9,true>", 8: "pik::ik_path_wide_kernel<9,8,true>",
                               16: "pik::ik_path_wide_kernel<9,16,true>"}),
    # (exact flavours, several tips: one lane per path whatever is asked for)
    (None, "torso_dual_arm", {1: "pik_exact::ik_path_kernel<9,true>", 16: "pik_exact::ik_path_kernel<9,true>"}),
], ids=["exact_panda", "fast_panda", "fast_two_tips", "exact_two_tips"])
def test_every_variant_returns_the_same_bits(O, exact, robot, lanes):
    ch = robots.by_name(robot)
    assert ch.dof == int(next(iter(lanes.values())).split("<")[1].split(",")[0])
    s = pk.Solver(ch, device=0, exact=exact)
    try:
        goals, start = (PR.straight_lines(ch, s.fk) if robot == "panda" else PR.joint_lines(ch, s.fk))
        p = pk.default_params(mode=1, minimal_displacement_weight=0.001)
        step = np.full(ch.dof, 0.1)
        P = len(start)
        ref = s.solve_paths(p, goals, start, step)  # the adaptive choice
        assert s.self_test(p, 32) == 0  # (no width switched off on this chain: a forced width is the width that runs)
        # (the cooperative kernels for several tips serve chains whose tips are all plain Denavit-Hartenberg ones: a
        #  handle they do not serve runs one lane per path whatever is asked for, and says so)
        served = robot == "panda" or exact is not False or "ik_path_wide_kernel" in s.path_kernel_name(p, 1)
        for l, name in lanes.items():
            s.set_option("lanes_per_elite", l)
            assert s.path_kernel_name(p, P) == (name if served else lanes[1])
            same(s.solve_paths(p, goals, start, step), ref, f"{robot} exact={exact} lanes {l}")
        s.set_option("lanes_per_elite", None)
        # one path: a team / cooperative kernel by default
        one = s.path_kernel_name(p, 1)
        if robot == "panda":
            assert "ik_path_team_kernel" in one or "ik_path_wide_kernel" in one, one
            assert one.endswith(",16>") or ",16," in one, one
        same(s.solve_paths(p, goals[:1], start[:1], step), [x[:1] for x in ref], f"{robot} exact={exact} one path")
        # ... and a call far too large for them: one lane per path
        assert "ik_path_kernel<" in s.path_kernel_name(p, 1 << 20)
    finally:
        s.close()


def test_strict_library_variants(O):
    ch = robots.panda()
    s = pk.Solver(ch, device=0, strict=True)
    try:
        goals, start = PR.straight_lines(ch, s.fk)
        p = pk.default_params(mode=1)
        ref = s.solve_paths(p, goals, start)
        for l, name in ((1, "pik_strict::ik_path_kernel<7,false>"), (4, "pik_strict::ik_path_team_kernel<7,4>"),
                        (16, "pik_strict::ik_path_team_kernel<7,16>")):
            s.set_option("lanes_per_elite", l)
            assert s.path_kernel_name(p, len(start)) == name
            same(s.solve_paths(p, goals, start), ref, f"strict lanes {l}")
    finally:
        s.close()


@pytest.mark.parametrize("limit", [None, 0.1])
def test_servo_paths_never_stop_on_a_solver_failure(O, exact_flavour, limit):
    """return_approximate_solution = 1 (servoing): every waypoint of an UNREACHABLE straight line returns the best
    configuration found (status APPROXIMATE), which is held -- only the step limit can stop such a path"""
    ch = robots.panda()
    o = O.Oracle(ch)
    s = pk.Solver(ch, device=0, strict=True)
    step = None if limit is None else np.full(ch.dof, limit)
    try:
        with O.math_mode("portable"):
            goals, start = PR.straight_lines(ch, o.fk)
            goals[:, :, :3] += 2.0 * goals[:, :1, :3] / np.linalg.norm(goals[:, :1, :3], axis=2, keepdims=True)  # 2 m further out
            po = O.default_params(mode=1, return_approximate_solution=1)
            want = PR.reference_paths(lambda g, sd: o.solve_batch(po, g, sd, num_threads=O.max_threads()), goals, start, step)
        got = s.solve_paths(pk.default_params(mode=1, return_approximate_solution=1), goals, start, step)
        same(got, want, f"servo [{exact_flavour}] limit {limit}")
        sol, st, cost, stats, reached = got
        assert not (st == pk.NO_IK_SOLUTION).any()
        assert (st[st > 0] == pk.APPROXIMATE).all()
        if limit is None:
            assert (reached == goals.shape[1]).all() and (st == pk.APPROXIMATE).all()
        else:
            assert ((st == pk.PATH_JUMP).sum(axis=1) <= 1).all()
    finally:
        s.close()


def test_device_entry_point_streams_and_slots():
    """solve_paths_device on a non-default stream equals the host-pointer call; two slots in flight on two streams
    equal their serial answers (own interpreter: torch allocates the buffers)"""
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "path_device_check.py")], cwd=ROOT,
                       capture_output=True, text=True, timeout=900)
    assert r.returncode == 0 and "path device check OK" in r.stdout, r.stdout[-2000:] + r.stderr[-3000:]


def test_edges_and_refusals(O):
    ch = robots.panda()
    s = pk.Solver(ch, device=0)
    L, h = s._L, s._h
    try:
        goals, start = PR.straight_lines(ch, s.fk, P=48, W=1)
        p = pk.default_params(mode=1)
        # one waypoint: a plain local-mode solve_batch
        sol, st, cost, stats, reached = s.solve_paths(p, goals, start)
        b = s.solve_batch(p, goals[:, 0], start)
        np.testing.assert_array_equal(sol[:, 0], b[0])
        np.testing.assert_array_equal(st[:, 0], b[1])
        np.testing.assert_array_equal(cost[:, 0], b[2])
        np.testing.assert_array_equal(stats[:, 0], b[3])
        np.testing.assert_array_equal(reached, (b[1] > 0).astype(np.int32))
        assert 0 < reached.sum() < len(reached)
        # no path: nothing to do
        e = s.solve_paths(p, np.zeros((0, 5, 7)), np.zeros((0, 7)))
        assert e[0].shape == (0, 5, 7) and e[1].shape == (0, 5) and e[4].shape == (0,)
        # the optional outputs may be NULL
        sol2 = np.empty_like(sol)
        st2 = np.empty_like(st)
        dp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int32)

        def raw(params, P, W, goal=goals, start_=start, solution=sol2, status=st2):
            ptr = lambda a, t: None if a is None else a.ctypes.data_as(t)
            return L.pikamd_solve_paths(h, C.byref(params), P, W, ptr(goal, dp), ptr(start_, dp), None, ptr(solution, dp),
                                        ptr(status, ip), None, None, None)

        assert raw(p, len(start), 1) == 0
        np.testing.assert_array_equal(sol2, sol)
        np.testing.assert_array_equal(st2, st)
        # refusals: PIKAMD_EINVAL (-1) and a message
        err = lambda: L.pikamd_last_error().decode()
        assert raw(pk.default_params(mode=0), len(start), 1) == -1 and "local mode" in err()
        assert raw(p, len(start), 0) == -1 and "W >= 1" in err()
        assert raw(p, -1, 1) == -1 and "P >= 0" in err()
        for missing in ("goal", "start_", "solution", "status"):
            assert raw(p, len(start), 1, **{missing: None}) == -1 and "must not be NULL" in err(), missing
        assert raw(p, 0, 1, goal=None, start_=None, solution=None, status=None) == 0
        assert L.pikamd_solve_paths_device(h, C.byref(p), 4, 1, None, None, None, None, None, None, None, None, None, 0) == -1
        assert L.pikamd_solve_paths_device(h, C.byref(p), 0, 1, None, None, None, None, None, None, None, None, None, 999) == -1
        assert "slot" in err()
        with pytest.raises(pk.PickIkAmdError, match="local mode"):
            s.solve_paths(pk.default_params(), goals, start)
        s.set_option("joint_layout", "soa")
        with pytest.raises(pk.PickIkAmdError, match="joint_layout soa"):
            s.solve_paths(p, goals, start)
        s.set_option("joint_layout", "aos")
        same(s.solve_paths(p, goals, start), (sol, st, cost, stats, reached), "after the refusals")
    finally:
        s.close()


def test_every_optional_array_may_be_absent(O):
    """P = 3 paths of W = 3 waypoints (odd row counts: the int32 arrays end off an 8-byte boundary): the call with
    every optional array, then with each one NULL in turn -- every array still given is the full call's, bit for bit
    (the step limit given is "no limit": leaving it out changes no answer)"""
    ch = robots.panda()
    s = pk.Solver(ch, device=0)
    try:
        goals, start = PR.straight_lines(ch, s.fk, P=3, W=3)
        p = pk.default_params(mode=1)
        full = A.check_optional_arrays(
            lambda a: A.solve_paths(s._L, s._h, p, 3, 3, a), lambda: A.path_arrays(s, goals, start, np.full(ch.dof, -1.0)),
            ("final_cost", "stats", "reached", "max_joint_step"), A.PATH_OUTPUTS)
        same([full[k] for k in A.PATH_OUTPUTS], s.solve_paths(p, goals, start), "binding")
    finally:
        s.close()


def test_cpp_host_mirror_paths():
    """tests/native/path_check.cpp: Solver::ik_gradient_paths against the C ABI call and the loop of batch calls"""
    import __graft_entry__ as g
    g.build()
    src = os.path.join(ROOT, "tests", "native", "path_check.cpp")
    exe = os.path.join(ROOT, "tests", "native", "path_check")
    lib_dir = os.path.join(ROOT, "pick_ik_amd")
    if not os.path.exists(exe) or os.path.getmtime(exe) < max(
            os.path.getmtime(src), os.path.getmtime(os.path.join(lib_dir, "host", "pick_ik_amd.hpp"))):
        subprocess.run(["g++", "-std=c++17", "-O1", "-pthread", "-Wall", "-Wextra", "-Werror", src, "-o", exe,
                        "-L" + lib_dir, "-lpick_ik_amd", "-Wl,-rpath," + lib_dir, "-Wl,-rpath,/opt/rocm/lib"], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "path C++ checks OK" in r.stdout, r.stdout + r.stderr


def test_one_call_beats_the_loop_of_round_trips(O):
    """One path of 32 waypoints (Panda, joint-space line, the default exact handle): one launch and two copies against
    32 dependent solve_batch round trips in the same process -- both warmed, alternated 21 times, medians of a host
    clock around calls that end synchronised.  The baseline is existing, unchanged code and no margin is added: a fused
    call that does not beat 32 round trips is a defect.  (Figures of a run: profiles/path_latency.txt.)"""
    ch = robots.panda()
    s = pk.Solver(ch, device=0)
    try:
        goals, start = PR.joint_lines(ch, s.fk, P=1, W=32)
        p = pk.default_params(mode=1)
        assert s.solve_paths(p, goals, start)[4][0] == 32  # (the whole path holds: both sides do the same work)
        paths, loop, _, _ = PR.time_paths_against_loop(s, p, goals, start, reps=21)
        print(f"P = 1, W = 32 [{s.path_kernel_name(p, 1)}]: solve_paths {paths * 1e3:.3f} ms, loop of 32 solve_batch "
              f"{loop * 1e3:.3f} ms, ratio {loop / paths:.2f}")
        assert paths < loop, (paths, loop)
    finally:
        s.close()
