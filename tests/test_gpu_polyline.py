"""computeCartesianPath through waypoints on the GPU (pikamd_cartesian_waypoints).

Its result is DEFINED by pikamd_cartesian_paths, segment after segment (include/pick_ik_amd.h;
tests/polyline_reference.py holds the loop), so everything here compares at tolerance zero: against the loop over the
CPU oracle for the exact builds (the poses from the library's host interpolation applied to the oracle's forward
kinematics), against the loop over the handle's own calls for the default and the fast flavour, every kernel variant
against every other.  tests/test_polyline_cpu.py shows that the fixtures reach every branch of the loop."""
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
from tests import polyline_reference as LR

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
S, W = LR.S_POLYLINES, LR.W_POLYLINES


@pytest.fixture(scope="module")
def O(oracle_mod):
    import __graft_entry__ as g
    g.build()
    return oracle_mod


def same(got, want, what=""):
    assert len(got) >= len(want)
    for x, y, w in zip(got, want, LR.NAMES):
        np.testing.assert_array_equal(x, y, err_msg=f"{what}: {w}")


_oracle_memo = {}


def oracle_loop(O, exact_flavour, key, ch, c, start, targets, w, n_targets, step, **kw):
    """the loop over the oracle in the math mode set: (the nine arrays, info); computed once per key"""
    key = (exact_flavour,) + key
    if key not in _oracle_memo:
        with O.math_mode("portable"):
            o = O.Oracle(ch)
            po = O.default_params(mode=1, **kw)
            strict = exact_flavour == "portable"
            _oracle_memo[key] = LR.reference_polyline(
                lambda g, sd: o.solve_batch(po, g, sd, num_threads=O.max_threads()), o.fk,
                lambda cc, a, t, ww: pk.interpolate_poses(cc, a, t, ww, strict=strict), c, start, targets, w, n_targets, step)
    return _oracle_memo[key]


def handle_loop(s, p, c, start, targets, w, n_targets, step):
    """the loop over the handle's own fk, interpolate_poses and solve_batch"""
    strict = s._L is pk.solver.lib(True)
    return LR.reference_polyline(lambda g, sd: s.solve_batch(p, g, sd), s.fk,
                                 lambda cc, a, t, ww: pk.interpolate_poses(cc, a, t, ww, strict=strict), c, start, targets, w,
                                 n_targets, step)


@pytest.mark.parametrize("limit", [None, 0.1])
def test_panda_polylines_equal_the_loop_over_the_oracle(O, exact_flavour, limit):
    ch = robots.panda()
    start, targets, n_targets = LR.polylines(ch)
    c = pk.Cartesian(**LR.POLYLINES)
    step = None if limit is None else np.full(ch.dof, limit)
    want, info = oracle_loop(O, exact_flavour, ("polylines", limit), ch, c, start, targets, W, n_targets, step)
    cl = LR.classes(want, info, W, S)
    for name, least in (LR.MINIMA if limit is None else LR.MINIMA_LIMITED).items():
        assert cl[name] >= least, (name, cl)
    s = pk.Solver(ch, device=0, strict=True)
    try:
        p = pk.default_params(mode=1)
        got = s.cartesian_waypoints(p, c, start, targets, W, n_targets, step)
        print(f"panda polylines [{exact_flavour}] limit {limit} {s.cartesian_waypoints_kernel_name(p, len(start))}: {cl}")
        same(got, want, f"panda polylines [{exact_flavour}] limit {limit}")
    finally:
        s.close()


def test_turning_equals_the_loop_over_the_oracle(O, exact_flavour):
    ch = robots.panda()
    c = pk.Cartesian(frame=1, max_rotation=0.05)
    with O.math_mode("portable"):
        start, targets = LR.turning(ch, O.Oracle(ch).fk)
    want, info = oracle_loop(O, exact_flavour, ("turning",), ch, c, start, targets, 24, None, None)
    cl = LR.classes(want, info, 24, 2)
    assert 1 <= cl["complete"] < len(start) and cl["moved_boundary"] >= 1, cl
    s = pk.Solver(ch, device=0, strict=True)
    try:
        same(s.cartesian_waypoints(pk.default_params(mode=1), c, start, targets, 24), want, f"turning [{exact_flavour}]")
    finally:
        s.close()


@pytest.mark.parametrize("robot", ["ur5", "panda_on_torso"])
def test_other_chain_lengths_equal_the_loop_over_the_oracle(O, exact_flavour, robot):
    ch = robots.by_name(robot)
    start, targets, n_targets = LR.polylines(ch, P=24)
    c = pk.Cartesian(**LR.POLYLINES)
    step = np.full(ch.dof, 0.2)
    want, info = oracle_loop(O, exact_flavour, (robot,), ch, c, start, targets, W, n_targets, step,
                             minimal_displacement_weight=0.001)
    cl = LR.classes(want, info, W, S)
    assert cl["complete"] + cl["relative_on_complete"] >= 1 and cl["no_fit_first"] + cl["no_fit_later"] >= 1, cl
    s = pk.Solver(ch, device=0, strict=True)
    try:
        got = s.cartesian_waypoints(pk.default_params(mode=1, minimal_displacement_weight=0.001), c, start, targets, W,
                                    n_targets, step)
        same(got, want, f"{robot} [{exact_flavour}] {cl}")
    finally:
        s.close()


@pytest.mark.parametrize("exact", [None, False], ids=["default_exact", "fast"])
def test_call_equals_the_loop_over_the_handles_own_calls(O, exact):
    ch = robots.panda()
    s = pk.Solver(ch, device=0, exact=exact)
    try:
        start, targets, n_targets = LR.polylines(ch)
        c = pk.Cartesian(**LR.POLYLINES)
        for kw, limit in (({}, None), (dict(minimal_displacement_weight=0.001), 0.1)):
            p = pk.default_params(mode=1, **kw)
            step = None if limit is None else np.full(ch.dof, limit)
            want, info = handle_loop(s, p, c, start, targets, W, n_targets, step)
            same(s.cartesian_waypoints(p, c, start, targets, W, n_targets, step), want, f"exact={exact} {kw} limit {limit}")
            cl = LR.classes(want, info, W, S)
            assert cl["complete"] >= 1 and cl["no_fit_later"] >= 1 and cl["no_room"] >= 1, (exact, kw, cl)
        start, targets = LR.turning(ch, s.fk)
        c = pk.Cartesian(frame=1, max_rotation=0.05, max_translation=0.02, jump_factor=1.5)
        p = pk.default_params(mode=1)
        want, _ = handle_loop(s, p, c, start, targets, 24, None, None)
        same(s.cartesian_waypoints(p, c, start, targets, 24), want, f"exact={exact} turning")
    finally:
        s.close()


@pytest.mark.parametrize("exact,strict,lanes", [
    (None, False, {1: "pik_exact::ik_polyline_kernel<7>", 4: "pik_exact::ik_polyline_team_kernel<7,4>",
                   16: "pik_exact::ik_polyline_team_kernel<7,16>"}),
    (False, False, {1: "pik::ik_polyline_kernel<7>", 8: "pik::ik_polyline_wide_kernel<7,8>",
                    16: "pik::ik_polyline_wide_kernel<7,16>"}),
    (None, True, {1: "pik_strict::ik_polyline_kernel<7>", 4: "pik_strict::ik_polyline_team_kernel<7,4>",
                  16: "pik_strict::ik_polyline_team_kernel<7,16>"}),
], ids=["exact", "fast", "strict"])
def test_every_variant_returns_the_same_bits(O, exact, strict, lanes):
    ch = robots.panda()
    s = pk.Solver(ch, device=0, exact=exact, strict=strict)
    try:
        start, targets, n_targets = LR.polylines(ch)
        c = pk.Cartesian(**LR.POLYLINES)
        p = pk.default_params(mode=1, minimal_displacement_weight=0.001)
        step = np.full(ch.dof, 0.1)
        P = len(start)
        ref = s.cartesian_waypoints(p, c, start, targets, W, n_targets, step)  # the adaptive choice
        for l, name in lanes.items():
            s.set_option("lanes_per_elite", l)
            assert s.cartesian_waypoints_kernel_name(p, P) == name
            same(s.cartesian_waypoints(p, c, start, targets, W, n_targets, step), ref, f"exact={exact} strict={strict} lanes {l}")
        s.set_option("lanes_per_elite", None)
        one = s.cartesian_waypoints_kernel_name(p, 1)  # one path: a team / cooperative kernel by default
        assert one.endswith(",16>") and ("team" in one or "wide" in one), one
        for q in (1, 3):  # (paths 1 and 3: no room for the last target; leaves the workspace)
            same(s.cartesian_waypoints(p, c, start[q:q + 1], targets[q:q + 1], W, n_targets[q:q + 1], step),
                 [x[q:q + 1] for x in ref], f"path {q} alone")
        assert "ik_polyline_kernel<" in s.cartesian_waypoints_kernel_name(p, 1 << 20)
    finally:
        s.close()


def test_reductions_to_existing_calls(O):
    ch = robots.panda()
    s = pk.Solver(ch, device=0)
    try:
        p = pk.default_params(mode=1)
        start, targets, _ = LR.polylines(ch, P=33)
        one = targets[:, :1]
        # one target, no relative test: pikamd_cartesian_paths, array for array
        c = pk.Cartesian(frame=2, max_translation=0.04, min_steps=2)
        got = s.cartesian_waypoints(p, c, start, one, W)
        same(got[:8], s.cartesian_paths(p, c, start, one[:, 0], W), "S = 1, no relative test")
        np.testing.assert_array_equal(got[8][:, 0], got[5])
        assert (got[5] > W).any() and (got[4] == got[5]).any()
        # ... with a relative test: equal once the minimum is given
        c = pk.Cartesian(frame=2, max_translation=0.04, min_steps=10, jump_factor=1.1)
        got = s.cartesian_waypoints(p, c, start, one, W)
        same(got[:8], s.cartesian_paths(p, c, start, one[:, 0], W), "S = 1, relative test, min_steps 10")
        assert (got[1] == pk.PATH_RELATIVE_JUMP).any()
        # ... and MoveIt's minimum for a waypoint list is 1, not 10
        c = pk.Cartesian(frame=2, max_translation=0.04, jump_factor=1.1)
        got = s.cartesian_waypoints(p, c, start, one, W)
        assert (got[5] < 10).any() and (s.cartesian_paths(p, c, start, one[:, 0], W)[5] >= 10).all()
        # no target: nothing at all
        z = s.cartesian_waypoints(p, c, start, targets, W, np.zeros(len(start), dtype=np.int32))
        np.testing.assert_array_equal(z[0], np.tile(start[:, None, :], (1, W, 1)))
        assert (z[1] == 0).all() and (z[2] == 0.0).all() and (z[3] == np.zeros((), dtype=STATS_DTYPE)).all()
        assert (z[4] == 0).all() and (z[5] == 0).all() and (z[6] == 0.0).all() and (z[7] == 0.0).all() and (z[8] == 0).all()
        # n_targets is clamped to 0..S
        wide = s.cartesian_waypoints(p, c, start, targets, W, np.full(len(start), 99, dtype=np.int32))
        same(wide, s.cartesian_waypoints(p, c, start, targets, W), "n_targets above S")
        same(s.cartesian_waypoints(p, c, start, targets, W, np.full(len(start), -5, dtype=np.int32)), z, "n_targets below 0")
        # no path: nothing to do
        e = s.cartesian_waypoints(p, c, np.zeros((0, 7)), np.zeros((0, 2, 7)), 5)
        assert e[0].shape == (0, 5, 7) and e[5].shape == (0,) and e[8].shape == (0, 2)
    finally:
        s.close()


def test_device_entry_point_streams_and_slots():
    """own interpreter: torch allocates the buffers (tests/polyline_device_check.py)"""
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "polyline_device_check.py")], cwd=ROOT,
                       capture_output=True, text=True, timeout=900)
    print(r.stdout[-1500:])
    assert r.returncode == 0 and "polyline device check OK" in r.stdout, r.stdout[-2000:] + r.stderr[-3000:]


def _pattern(P, dof, w=W, s_=S):
    stats = np.full(P * w * STATS_DTYPE.itemsize, 0xAB, dtype=np.uint8).view(STATS_DTYPE).reshape(P, w)
    return dict(solution=np.full((P, w, dof), -7.5), status=np.full((P, w), -77, dtype=np.int32),
                final_cost=np.full((P, w), -7.5), stats=stats, reached=np.full(P, -77, dtype=np.int32),
                steps=np.full(P, -77, dtype=np.int32), segment_steps=np.full((P, s_), -77, dtype=np.int32),
                fraction=np.full(P, -7.5), goals=np.full((P, w, 7), -7.5))


ORDER = ("solution", "status", "final_cost", "stats", "reached", "steps", "fraction", "goals", "segment_steps")


def _raw(s, p, c, start, targets, n_targets, step, a, P=None, s_=S, w=W):
    """pikamd_cartesian_waypoints as the C ABI takes it (tests/abi_calls.py); a: the outputs"""
    return A.cartesian_waypoints(s._L, s._h, p, c, len(start) if P is None else P, s_, w,
                                 dict(a, start=start, targets=targets, n_targets=n_targets, max_joint_step=step))


def test_every_optional_array_may_be_absent(O):
    """P = 5 paths of W = 16 rows and S = 3 targets (odd counts: the int32 arrays end off an 8-byte boundary): the
    call with every array, then with each optional one NULL in turn -- every array still given is the full call's, bit
    for bit (the step limit given is "no limit" and n_targets is S: leaving them out changes no answer)"""
    ch = robots.panda()
    s = pk.Solver(ch, device=0)
    try:
        start, targets, _ = LR.polylines(ch, P=5)
        c = pk.Cartesian(**LR.POLYLINES)
        p = pk.default_params(mode=1)
        none, every = np.full(ch.dof, -1.0), np.full(5, S, dtype=np.int32)
        full = _pattern(5, ch.dof)
        assert _raw(s, p, c, start, targets, every, none, full) == 0
        for k in ORDER:
            assert full[k].tobytes() != _pattern(5, ch.dof)[k].tobytes(), f"{k} was not written"
            poison = np.frombuffer(_pattern(5, ch.dof)[k].tobytes(), dtype=np.uint8)
            left = np.frombuffer(full[k].tobytes(), dtype=np.uint8).reshape(-1, full[k].dtype.itemsize)
            assert not (left == poison.reshape(left.shape)).all(axis=1).any(), f"{k}: an element was left as it was"
        for gone in ("final_cost", "stats", "reached", "segment_steps", "fraction", "goals", "max_joint_step", "n_targets"):
            a = _pattern(5, ch.dof)
            if gone in a:
                a[gone] = None
            rc = _raw(s, p, c, start, targets, None if gone == "n_targets" else every,
                      None if gone == "max_joint_step" else none, a)
            assert rc == 0, gone
            for k in ORDER:
                if a[k] is not None:
                    assert a[k].tobytes() == full[k].tobytes(), f"without {gone}: {k} differs"
        same([full[k] for k in ORDER], s.cartesian_waypoints(p, c, start, targets, W), "binding")
        lean = s.cartesian_waypoints(p, c, start, targets, W, optional=False)
        np.testing.assert_array_equal(lean[0], full["solution"])
        np.testing.assert_array_equal(lean[5], full["steps"])
        assert lean[2] is None and lean[7] is None and lean[8] is None
    finally:
        s.close()


def test_refusals(O):
    ch = robots.panda()
    s = pk.Solver(ch, device=0)
    L = s._L
    try:
        start, targets, n_targets = LR.polylines(ch, P=4)
        c = pk.Cartesian(**LR.POLYLINES)
        p = pk.default_params(mode=1)
        err = lambda: L.pikamd_last_error().decode()
        a = _pattern(4, ch.dof)
        assert _raw(s, p, c, start, targets, n_targets, None, a) == 0
        # PIKAMD_EINVAL (-1) and a message
        assert _raw(s, pk.default_params(mode=0), c, start, targets, n_targets, None, a) == -1 and "local mode" in err()
        assert _raw(s, None, c, start, targets, n_targets, None, a) == -1
        assert _raw(s, p, None, start, targets, n_targets, None, a) == -1 and "pikamd_cartesian" in err()
        assert _raw(s, p, c, start, targets, n_targets, None, a, w=0) == -1 and "W >= 1" in err()
        assert _raw(s, p, c, start, targets, n_targets, None, a, P=-1) == -1 and "P >= 0" in err()
        assert _raw(s, p, c, start, targets, n_targets, None, a, s_=0) == -1 and "S >= 1" in err()
        assert _raw(s, p, c, start, targets, n_targets, None, a, s_=3, w=2) == -1 and "S <= W" in err()
        assert _raw(s, p, c, start, targets, n_targets, None, dict(a, steps=None)) == -1 and "steps" in err()
        assert _raw(s, p, c, start, targets, n_targets, None, dict(a, steps=None), P=0) == -1  # (required whatever P)
        for missing in ("solution", "status"):
            assert _raw(s, p, c, start, targets, n_targets, None, dict(a, **{missing: None})) == -1 and "must not be NULL" in err(), missing
        assert _raw(s, p, c, None, targets, n_targets, None, a, P=4) == -1 and "must not be NULL" in err()
        assert _raw(s, p, c, start, None, n_targets, None, a, P=4) == -1 and "targets" in err()
        assert _raw(s, p, c, None, None, None, None, dict(a, solution=None, status=None), P=0) == 0
        for bad, word in ((dict(frame=3), "frame"), (dict(frame=-1), "frame"), (dict(min_steps=-1), "min_steps"),
                          (dict(max_translation=0.0, max_rotation=0.0), "neither"),
                          (dict(max_translation=float("nan"), max_rotation=-1.0), "neither")):
            cc = pk.Cartesian(**dict(LR.POLYLINES, **bad))
            assert _raw(s, p, cc, start, targets, n_targets, None, a) == -1 and word in err(), bad
        args = (None,) * 13
        assert L.pikamd_cartesian_waypoints_device(s._h, C.byref(p), C.byref(c), 4, S, W, *args, None, 0) == -1
        assert L.pikamd_cartesian_waypoints_device(s._h, C.byref(p), C.byref(c), 0, S, W, None, None, None, None, None, None,
                                                   None, None, None, 1, None, None, None, None, 999) == -1
        assert "slot" in err()
        s.set_option("joint_layout", "soa")
        with pytest.raises(pk.PickIkAmdError, match="joint_layout soa"):
            s.cartesian_waypoints(p, c, start, targets, W)
        s.set_option("joint_layout", "aos")
        b = _pattern(4, ch.dof)
        assert _raw(s, p, c, start, targets, n_targets, None, b) == 0
        for k in ORDER:
            assert a[k].tobytes() == b[k].tobytes(), k  # (after the refusals: the first call's answers)
    finally:
        s.close()
    # several tip frames: PIKAMD_EUNSUPPORTED (-4)
    ch2 = robots.torso_dual_arm()
    s2 = pk.Solver(ch2, device=0)
    try:
        call = lambda: s2.cartesian_waypoints(pk.default_params(mode=1), pk.Cartesian(**LR.POLYLINES), np.zeros((2, ch2.dof)),
                                              np.zeros((2, 2, 7)), 4)
        with pytest.raises(pk.PickIkAmdError, match="tip frames"):
            call()
        assert "error -4" in str(pytest.raises(pk.PickIkAmdError, call).value)
    finally:
        s2.close()


def test_cpp_host_mirror():
    """tests/native/polyline_check.cpp: Solver::compute_cartesian_waypoints against the C ABI call"""
    import __graft_entry__ as g
    g.build()
    src = os.path.join(ROOT, "tests", "native", "polyline_check.cpp")
    exe = os.path.join(ROOT, "tests", "native", "polyline_check")
    lib_dir = os.path.join(ROOT, "pick_ik_amd")
    if not os.path.exists(exe) or os.path.getmtime(exe) < max(
            os.path.getmtime(src), os.path.getmtime(os.path.join(lib_dir, "host", "pick_ik_amd.hpp"))):
        subprocess.run(["g++", "-std=c++17", "-O1", "-pthread", "-Wall", "-Wextra", "-Werror", src, "-o", exe,
                        "-L" + lib_dir, "-lpick_ik_amd", "-Wl,-rpath," + lib_dir, "-Wl,-rpath,/opt/rocm/lib"], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "polyline C++ checks OK" in r.stdout, r.stdout + r.stderr
