"""computeCartesianPath in one call on the GPU (pikamd_cartesian_paths).

Its result is DEFINED by pikamd_fk_batch, pikamd_interpolate_poses and pikamd_solve_paths (include/pick_ik_amd.h;
tests/cartesian_reference.py holds the loop), so everything here compares at tolerance zero: against the loop over the
CPU oracle for the exact builds (the poses from the library's host interpolation applied to the oracle's forward
kinematics), against the loop over the handle's own calls for the default and the fast flavour, every kernel variant
against every other.  tests/test_cartesian_cpu.py shows that the fixtures reach every branch of the loop."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import pick_ik_amd as pk
from pick_ik_amd import robots
from pick_ik_amd.solver import STATS_DTYPE
from tests import abi_calls as A
from tests import cartesian_reference as CR

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = CR.NAMES + ("goals",)
W = 12


@pytest.fixture(scope="module")
def O(oracle_mod):
    import __graft_entry__ as g
    g.build()
    return oracle_mod


def same(got, want, what=""):
    assert len(got) >= len(want)
    for x, y, w in zip(got, want, NAMES):
        np.testing.assert_array_equal(x, y, err_msg=f"{what}: {w}")


def oracle_loop(O, exact_flavour, ch, c, start, target, w, step, **kw):
    """the loop over the oracle in the math mode set: (the seven arrays and the poses, held)"""
    o = O.Oracle(ch)
    goals, steps = pk.interpolate_poses(c, o.fk(start), target, w, strict=exact_flavour == "portable")
    po = O.default_params(mode=1, **kw)
    out, held = CR.reference_cartesian(lambda g, sd: o.solve_batch(po, g, sd, num_threads=O.max_threads()), goals, steps,
                                       start, c.jump_factor, step)
    return out + (goals,), held


def handle_loop(s, p, c, start, target, w, step):
    """the loop over the handle's own fk, interpolate_poses and solve_batch"""
    goals, steps = pk.interpolate_poses(c, s.fk(start), target, w, strict=s._L is pk.solver.lib(True))
    out, held = CR.reference_cartesian(lambda g, sd: s.solve_batch(p, g, sd), goals, steps, start, c.jump_factor, step)
    return out + (goals,), held


@pytest.mark.parametrize("limit", [None, 0.1])
def test_panda_offsets_equal_the_loop_over_the_oracle(O, exact_flavour, limit):
    ch = robots.panda()
    start, target = CR.offsets(ch)
    c = pk.Cartesian(**CR.OFFSETS)
    step = None if limit is None else np.full(ch.dof, limit)
    with O.math_mode("portable"):
        want, held = oracle_loop(O, exact_flavour, ch, c, start, target, W, step)
    cl = CR.classes(want[:7], held, W)
    assert min(cl[0], cl[1], cl[3], cl[4]) >= 4 and (limit is None or cl[2] >= 4) and (limit is not None or cl[5] >= 1), cl
    s = pk.Solver(ch, device=0, strict=True)
    try:
        p = pk.default_params(mode=1)
        got = s.cartesian_paths(p, c, start, target, W, step)
        print(f"panda offsets [{exact_flavour}] limit {limit} {s.cartesian_kernel_name(p, len(start))}: complete / "
              f"solver / absolute / relative / too long / relative on complete = {cl}")
        same(got, want, f"panda offsets [{exact_flavour}] limit {limit}")
    finally:
        s.close()


@pytest.mark.parametrize("frame", [0, 1], ids=["global", "tip"])
def test_rotating_targets_equal_the_loop_over_the_oracle(O, exact_flavour, frame):
    ch = robots.panda()
    c = pk.Cartesian(frame=frame, max_rotation=0.05, min_steps=3)
    with O.math_mode("portable"):
        start, target = CR.rotating(ch, O.Oracle(ch).fk, frame)
        want, held = oracle_loop(O, exact_flavour, ch, c, start, target, 16, None)
    cl = CR.classes(want[:7], held, 16)
    assert cl[0] >= 1 and cl[1] + cl[4] >= 1, cl
    s = pk.Solver(ch, device=0, strict=True)
    try:
        same(s.cartesian_paths(pk.default_params(mode=1), c, start, target, 16), want, f"rotating frame {frame} [{exact_flavour}]")
    finally:
        s.close()


@pytest.mark.parametrize("robot", ["ur5", "panda_on_torso"])
def test_other_chain_lengths_equal_the_loop_over_the_oracle(O, exact_flavour, robot):
    ch = robots.by_name(robot)
    start, target = CR.offsets(ch, P=24)
    c = pk.Cartesian(**CR.OFFSETS)
    step = np.full(ch.dof, 0.2)
    with O.math_mode("portable"):
        want, held = oracle_loop(O, exact_flavour, ch, c, start, target, W, step, minimal_displacement_weight=0.001)
    cl = CR.classes(want[:7], held, W)
    assert cl[0] + cl[3] >= 1 and cl[4] >= 1, cl
    s = pk.Solver(ch, device=0, strict=True)
    try:
        got = s.cartesian_paths(pk.default_params(mode=1, minimal_displacement_weight=0.001), c, start, target, W, step)
        same(got, want, f"{robot} [{exact_flavour}] {cl}")
    finally:
        s.close()


@pytest.mark.parametrize("exact", [None, False], ids=["default_exact", "fast"])
def test_call_equals_the_loop_over_the_handles_own_calls(O, exact):
    ch = robots.panda()
    s = pk.Solver(ch, device=0, exact=exact)
    try:
        start, target = CR.offsets(ch)
        c = pk.Cartesian(**CR.OFFSETS)
        for kw, limit in (({}, None), (dict(minimal_displacement_weight=0.001), 0.1)):
            p = pk.default_params(mode=1, **kw)
            step = None if limit is None else np.full(ch.dof, limit)
            want, held = handle_loop(s, p, c, start, target, W, step)
            same(s.cartesian_paths(p, c, start, target, W, step), want, f"exact={exact} {kw} limit {limit}")
            cl = CR.classes(want[:7], held, W)
            assert cl[0] >= 1 and cl[1] + cl[2] >= 1 and cl[3] >= 1 and cl[4] >= 1, (exact, kw, cl)
        # a rotating target in the tip frame as well
        start, target = CR.rotating(ch, s.fk, 1)
        c = pk.Cartesian(frame=1, max_rotation=0.05, max_translation=0.02, jump_factor=1.5)
        p = pk.default_params(mode=1)
        want, _ = handle_loop(s, p, c, start, target, 16, None)
        same(s.cartesian_paths(p, c, start, target, 16), want, f"exact={exact} rotating")
        assert (want[5] >= 10).all()
    finally:
        s.close()


@pytest.mark.parametrize("exact,strict,lanes", [
    (None, False, {1: "pik_exact::ik_cartesian_kernel<7>", 4: "pik_exact::ik_cartesian_team_kernel<7,4>",
                   16: "pik_exact::ik_cartesian_team_kernel<7,16>"}),
    (False, False, {1: "pik::ik_cartesian_kernel<7>", 8: "pik::ik_cartesian_wide_kernel<7,8>",
                    16: "pik::ik_cartesian_wide_kernel<7,16>"}),
    (None, True, {1: "pik_strict::ik_cartesian_kernel<7>", 4: "pik_strict::ik_cartesian_team_kernel<7,4>",
                  16: "pik_strict::ik_cartesian_team_kernel<7,16>"}),
], ids=["exact", "fast", "strict"])
def test_every_variant_returns_the_same_bits(O, exact, strict, lanes):
    ch = robots.panda()
    s = pk.Solver(ch, device=0, exact=exact, strict=strict)
    try:
        start, target = CR.offsets(ch)
        c = pk.Cartesian(**CR.OFFSETS)
        p = pk.default_params(mode=1, minimal_displacement_weight=0.001)
        step = np.full(ch.dof, 0.1)
        P = len(start)
        ref = s.cartesian_paths(p, c, start, target, W, step)  # the adaptive choice
        for l, name in lanes.items():
            s.set_option("lanes_per_elite", l)
            assert s.cartesian_kernel_name(p, P) == name
            same(s.cartesian_paths(p, c, start, target, W, step), ref, f"exact={exact} strict={strict} lanes {l}")
        s.set_option("lanes_per_elite", None)
        one = s.cartesian_kernel_name(p, 1)  # one path: a team / cooperative kernel by default
        assert one.endswith(",16>") and ("team" in one or "wide" in one), one
        same(s.cartesian_paths(p, c, start[:1], target[:1], W, step), [x[:1] for x in ref], "one path")
        assert "ik_cartesian_kernel<" in s.cartesian_kernel_name(p, 1 << 20)
    finally:
        s.close()


def test_reductions_to_existing_calls(O):
    ch = robots.panda()
    s = pk.Solver(ch, device=0)
    try:
        p = pk.default_params(mode=1)
        start, target = CR.offsets(ch, P=33)
        # every path the same number of steps: min_steps = W above every floor -- fk + interpolate_poses + solve_paths
        c = pk.Cartesian(frame=2, max_translation=0.1, min_steps=8)
        sol, st, cost, stats, reached, steps, fraction, goals = s.cartesian_paths(p, c, start, target, 8)
        assert (steps == 8).all()
        g, n = pk.interpolate_poses(c, s.fk(start), target, 8)
        np.testing.assert_array_equal(goals, g)
        np.testing.assert_array_equal(steps, n)
        same((sol, st, cost, stats, reached), s.solve_paths(p, g, start), "solve_paths")
        np.testing.assert_array_equal(fraction, reached / 8.0)
        assert 0 < (reached == 8).sum() < len(reached)
        # MoveIt's minimum with a relative test: at least 10 steps
        c = pk.Cartesian(frame=2, max_translation=0.1, jump_factor=4.0)
        out = s.cartesian_paths(p, c, start, target, 10)
        assert (out[5] >= 10).all() and (out[5] == 10).any() and (out[5] > 10).sum() == 0
        # no path: nothing to do
        e = s.cartesian_paths(p, c, np.zeros((0, 7)), np.zeros((0, 7)), 5)
        assert e[0].shape == (0, 5, 7) and e[5].shape == (0,)
    finally:
        s.close()


def test_device_entry_point_streams_and_slots():
    """own interpreter: torch allocates the buffers (tests/cartesian_device_check.py)"""
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "cartesian_device_check.py")], cwd=ROOT,
                       capture_output=True, text=True, timeout=900)
    assert r.returncode == 0 and "cartesian device check OK" in r.stdout, r.stdout[-2000:] + r.stderr[-3000:]


def _pattern(P, dof):
    stats = np.full(P * W * STATS_DTYPE.itemsize, 0xAB, dtype=np.uint8).view(STATS_DTYPE).reshape(P, W)
    return dict(solution=np.full((P, W, dof), -7.5), status=np.full((P, W), -77, dtype=np.int32),
                final_cost=np.full((P, W), -7.5), stats=stats, reached=np.full(P, -77, dtype=np.int32),
                steps=np.full(P, -77, dtype=np.int32), fraction=np.full(P, -7.5), goals=np.full((P, W, 7), -7.5))


ORDER = ("solution", "status", "final_cost", "stats", "reached", "steps", "fraction", "goals")


def _raw(s, p, c, start, target, step, a, P=None, w=W):
    """pikamd_cartesian_paths as the C ABI takes it (tests/abi_calls.py); a: the outputs"""
    return A.cartesian_paths(s._L, s._h, p, c, len(start) if P is None else P, w,
                             dict(a, start=start, target=target, max_joint_step=step))


def test_every_optional_array_may_be_absent(O):
    """P = 5 paths of W = 12 rows (odd counts: the int32 arrays end off an 8-byte boundary): the call with every array,
    then with each optional one NULL in turn -- every array still given is the full call's, bit for bit (the step
    limit given is "no limit": leaving it out changes no answer)"""
    ch = robots.panda()
    s = pk.Solver(ch, device=0)
    try:
        start, target = CR.offsets(ch, P=5)
        c = pk.Cartesian(**CR.OFFSETS)
        p = pk.default_params(mode=1)
        none = np.full(ch.dof, -1.0)
        full = _pattern(5, ch.dof)
        assert _raw(s, p, c, start, target, none, full) == 0
        for k in ORDER:
            assert full[k].tobytes() != _pattern(5, ch.dof)[k].tobytes(), f"{k} was not written"
        for gone in ("final_cost", "stats", "reached", "fraction", "goals", "max_joint_step"):
            a = _pattern(5, ch.dof)
            if gone != "max_joint_step":
                a[gone] = None
            assert _raw(s, p, c, start, target, None if gone == "max_joint_step" else none, a) == 0, gone
            for k in ORDER:
                if a[k] is not None:
                    assert a[k].tobytes() == full[k].tobytes(), f"without {gone}: {k} differs"
        same([full[k] for k in ORDER], s.cartesian_paths(p, c, start, target, W), "binding")
        lean = s.cartesian_paths(p, c, start, target, W, optional=False)
        np.testing.assert_array_equal(lean[0], full["solution"])
        np.testing.assert_array_equal(lean[5], full["steps"])
        assert lean[2] is None and lean[7] is None
    finally:
        s.close()


def test_refusals(O):
    ch = robots.panda()
    s = pk.Solver(ch, device=0)
    L = s._L
    try:
        start, target = CR.offsets(ch, P=4)
        c = pk.Cartesian(**CR.OFFSETS)
        p = pk.default_params(mode=1)
        err = lambda: L.pikamd_last_error().decode()
        a = _pattern(4, ch.dof)
        assert _raw(s, p, c, start, target, None, a) == 0
        # PIKAMD_EINVAL (-1) and a message
        assert _raw(s, pk.default_params(mode=0), c, start, target, None, a) == -1 and "local mode" in err()
        assert _raw(s, None, c, start, target, None, a) == -1
        assert _raw(s, p, None, start, target, None, a) == -1 and "pikamd_cartesian" in err()
        assert _raw(s, p, c, start, target, None, a, w=0) == -1 and "W >= 1" in err()
        assert _raw(s, p, c, start, target, None, a, P=-1) == -1 and "P >= 0" in err()
        assert _raw(s, p, c, start, target, None, dict(a, steps=None)) == -1 and "steps" in err()
        assert _raw(s, p, c, start, target, None, dict(a, steps=None), P=0) == -1  # (required whatever P)
        for missing in ("solution", "status"):
            assert _raw(s, p, c, start, target, None, dict(a, **{missing: None})) == -1 and "must not be NULL" in err(), missing
        assert _raw(s, p, c, None, target, None, a, P=4) == -1 and "must not be NULL" in err()
        assert _raw(s, p, c, start, None, None, a, P=4) == -1 and "must not be NULL" in err()
        assert _raw(s, p, c, None, None, None, dict(a, solution=None, status=None), P=0) == 0
        for bad, word in ((dict(frame=3), "frame"), (dict(frame=-1), "frame"), (dict(min_steps=-1), "min_steps"),
                          (dict(max_translation=0.0, max_rotation=0.0), "neither"),
                          (dict(max_translation=float("nan"), max_rotation=-1.0), "neither")):
            cc = pk.Cartesian(**dict(CR.OFFSETS, **bad))
            assert _raw(s, p, cc, start, target, None, a) == -1 and word in err(), bad
        args = (None,) * 11
        assert L.pikamd_cartesian_paths_device(s._h, C.byref(p), C.byref(c), 4, W, *args, None, 0) == -1
        assert L.pikamd_cartesian_paths_device(s._h, C.byref(p), C.byref(c), 0, W, None, None, None, None, None, None, None,
                                               None, 1, None, None, None, 999) == -1
        assert "slot" in err()
        s.set_option("joint_layout", "soa")
        with pytest.raises(pk.PickIkAmdError, match="joint_layout soa"):
            s.cartesian_paths(p, c, start, target, W)
        s.set_option("joint_layout", "aos")
        b = _pattern(4, ch.dof)
        assert _raw(s, p, c, start, target, None, b) == 0
        for k in ORDER:
            assert a[k].tobytes() == b[k].tobytes(), k  # (after the refusals: the first call's answers)
    finally:
        s.close()
    # several tip frames: PIKAMD_EUNSUPPORTED (-4)
    ch2 = robots.torso_dual_arm()
    s2 = pk.Solver(ch2, device=0)
    try:
        with pytest.raises(pk.PickIkAmdError, match="tip frames"):
            s2.cartesian_paths(pk.default_params(mode=1), pk.Cartesian(**CR.OFFSETS), np.zeros((2, ch2.dof)), np.zeros((2, 7)), 4)
        assert "error -4" in str(pytest.raises(pk.PickIkAmdError, s2.cartesian_paths, pk.default_params(mode=1),
                                               pk.Cartesian(**CR.OFFSETS), np.zeros((2, ch2.dof)), np.zeros((2, 7)), 4).value)
    finally:
        s2.close()


def test_cpp_host_mirror():
    """tests/native/cartesian_check.cpp: Solver::compute_cartesian_paths against the C ABI call and the host
    interpolation"""
    import __graft_entry__ as g
    g.build()
    src = os.path.join(ROOT, "tests", "native", "cartesian_check.cpp")
    exe = os.path.join(ROOT, "tests", "native", "cartesian_check")
    lib_dir = os.path.join(ROOT, "pick_ik_amd")
    if not os.path.exists(exe) or os.path.getmtime(exe) < max(
            os.path.getmtime(src), os.path.getmtime(os.path.join(lib_dir, "host", "pick_ik_amd.hpp"))):
        subprocess.run(["g++", "-std=c++17", "-O1", "-pthread", "-Wall", "-Wextra", "-Werror", src, "-o", exe,
                        "-L" + lib_dir, "-lpick_ik_amd", "-Wl,-rpath," + lib_dir, "-Wl,-rpath,/opt/rocm/lib"], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "cartesian C++ checks OK" in r.stdout, r.stdout + r.stderr
