"""computeCartesianPath through waypoints (CPU): the normative loop of pikamd_cartesian_waypoints
(tests/polyline_reference.py) over the CPU oracle on the fixtures of the GPU tests -- each must reach every class, so
that the GPU comparison (tests/test_gpu_polyline.py) cannot pass on one branch only --, the shape of the rows behind
every kind of stop with the fraction recomputed independently, the declarations, the shape checks, the build tables and
the resource ledger of the new kernels."""
import csv
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from tests import cartesian_reference as CR
from tests import path_reference as PR
from tests import polyline_reference as LR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("pikamd_cartesian_waypoints", "pikamd_cartesian_waypoints_device", "pikamd_cartesian_waypoints_kernel_name")
S, W = LR.S_POLYLINES, LR.W_POLYLINES


@pytest.fixture(params=["portable", "fma"])
def mode(request):
    return request.param


@pytest.fixture(scope="module")
def pk():
    import __graft_entry__ as g
    g.build()
    import pick_ik_amd
    return pick_ik_amd


# ---- the normative loop over the oracle -------------------------------------------------------------
_memo = {}


def oracle_polylines(O, pk, mode, limit):
    """the fixture "panda polylines" through the loop over the oracle in one math mode (the poses by the host
    interpolation of the library that goes with it); computed once per (mode, limit)"""
    if (mode, limit) not in _memo:
        ch = pk.robots.panda()
        start, targets, n_targets = LR.polylines(ch)
        step = None if limit is None else np.full(ch.dof, limit)
        with O.math_mode(mode):
            o = O.Oracle(ch)
            po = O.default_params(mode=1)
            strict = mode == "portable"
            out, info = LR.reference_polyline(
                lambda g, sd: o.solve_batch(po, g, sd, num_threads=O.max_threads()), o.fk,
                lambda c, a, t, w: pk.interpolate_poses(c, a, t, w, strict=strict), pk.Cartesian(**LR.POLYLINES), start,
                targets, W, n_targets, step)
        _memo[(mode, limit)] = (start, targets, n_targets, out, info)
    return _memo[(mode, limit)]


def test_fixture_reaches_every_class(oracle_mod, pk, mode):
    free = oracle_polylines(oracle_mod, pk, mode, None)
    lim = oracle_polylines(oracle_mod, pk, mode, 0.1)
    cf, cl = LR.classes(free[3], free[4], W, S), LR.classes(lim[3], lim[4], W, S)
    print(f"panda polylines [{mode}]: no limit {cf}\n  limit 0.1 {cl}")
    for name, least in LR.MINIMA.items():
        assert cf[name] >= least, (name, cf)
    for name, least in LR.MINIMA_LIMITED.items():
        assert cl[name] >= least, (name, cl)
    assert cf["absolute_later"] == 0


def test_turning_fixture_has_both_branches(oracle_mod, pk, mode):
    O = oracle_mod
    ch = pk.robots.panda()
    with O.math_mode(mode):
        o = O.Oracle(ch)
        start, targets = LR.turning(ch, o.fk)
        po = O.default_params(mode=1)
        out, info = LR.reference_polyline(
            lambda g, sd: o.solve_batch(po, g, sd, num_threads=O.max_threads()), o.fk,
            lambda c, a, t, w: pk.interpolate_poses(c, a, t, w, strict=mode == "portable"),
            pk.Cartesian(frame=1, max_rotation=0.05), start, targets, 24)
    cl = LR.classes(out, info, 24, 2)
    print(f"turning [{mode}] steps {out[5].min()}..{out[5].max()}: {cl}")
    assert len(start) == 20 and cl["complete"] >= 1 and cl["complete"] < 20, cl
    assert cl["moved_boundary"] >= 1, cl  # (in the tip frame the second target hangs on the state reached)


@pytest.mark.parametrize("limit", [None, 0.1])
def test_row_shape_behind_every_kind_of_stop(oracle_mod, pk, mode, limit):
    start, targets, n_targets, out, info = oracle_polylines(oracle_mod, pk, mode, limit)
    sol, st, cost, stats, reached, steps, fraction, goals, segs = out
    zero = np.zeros((), dtype=PR.STATS_DTYPE)
    factor = LR.POLYLINES["jump_factor"]
    for p in range(len(start)):
        sp, r, held = int(n_targets[p]), int(reached[p]), int(info["held"][p])
        started = int((segs[p] > 0).sum())
        assert (segs[p, :started] >= LR.POLYLINES["min_steps"]).all() and (segs[p, started:] == 0).all() and started <= sp
        assert int(segs[p].sum()) == steps[p]  # (the rows of every segment started)
        assert (st[p, :r] > 0).all() and 0 <= r <= held <= min(int(steps[p]), W)
        last = sol[p, r - 1] if r > 0 else start[p]
        # the fraction, from the segment counts alone: the complete segments, then the share of the one it stopped in
        done, rows = 0, 0
        while done < started and rows + segs[p, done] <= held and rows + segs[p, done] <= W:
            rows += int(segs[p, done])
            done += 1
        want = np.float64(done) / np.float64(sp)
        if done < started and rows + segs[p, done] <= W:  # (stopped inside a segment that fitted)
            want = want + (np.float64(held - rows) / np.float64(segs[p, done])) / np.float64(sp)
        relative = r < W and st[p, r] == pk.PATH_RELATIVE_JUMP
        if relative:
            want = want * (np.float64(r + 1) / np.float64(held + 1))
            assert stats["cost_evals"][p, r] > 0 and factor > 0.0  # (its counters stay)
        else:
            assert r == held
        assert fraction[p] == want, (p, fraction[p], want, segs[p], held)
        # the rows behind the stop
        fitted = steps[p] <= W
        whole = fitted and held == steps[p] and started == sp
        behind = r if (whole and not relative) or (not fitted and not relative and held == rows) else r + 1
        if behind > r:
            assert st[p, r] in (pk.NO_IK_SOLUTION, pk.PATH_JUMP, pk.PATH_RELATIVE_JUMP), (p, st[p, r])
            np.testing.assert_array_equal(sol[p, r], last)
        assert (st[p, behind:] == CR.NOT_ATTEMPTED).all() and (cost[p, behind:] == 0.0).all()
        assert (stats[p, behind:] == zero).all()
        np.testing.assert_array_equal(sol[p, behind:], np.tile(last, (W - behind, 1)))
        if whole and not relative:
            assert fraction[p] == 1.0


def test_no_target_and_one_target(oracle_mod, pk):
    """n_targets = 0 is nothing at all; S = 1 without a relative test is the loop of pikamd_cartesian_paths"""
    O = oracle_mod
    ch = pk.robots.panda()
    start, targets, _ = LR.polylines(ch, P=12)
    with O.math_mode("portable"):
        o = O.Oracle(ch)
        po = O.default_params(mode=1)
        solve = lambda g, sd: o.solve_batch(po, g, sd, num_threads=O.max_threads())
        interp = lambda c, a, t, w: pk.interpolate_poses(c, a, t, w, strict=True)
        c = pk.Cartesian(frame=2, max_translation=0.04, min_steps=2)
        out, _ = LR.reference_polyline(solve, o.fk, interp, c, start, targets, W, np.zeros(12, dtype=np.int32))
        assert (out[4] == 0).all() and (out[5] == 0).all() and (out[6] == 0.0).all() and (out[8] == 0).all()
        assert (out[1] == 0).all() and (out[7] == 0.0).all()
        np.testing.assert_array_equal(out[0], np.tile(start[:, None, :], (1, W, 1)))
        one, _ = LR.reference_polyline(solve, o.fk, interp, c, start, targets[:, :1], W)
        goals, steps = interp(c, o.fk(start), targets[:, 0], W)
        want, _ = CR.reference_cartesian(solve, goals, steps, start)
        for x, y, name in zip(one, want + (goals,), LR.NAMES):
            np.testing.assert_array_equal(x, y, err_msg=name)
        np.testing.assert_array_equal(one[8][:, 0], steps)


# ---- declarations, bindings, build ----------------------------------------------------------------
def test_header_and_bindings_declare_the_entry_points(pk):
    header = open(os.path.join(ROOT, "include", "pick_ik_amd.h")).read()
    begin, end = header.index("[host-api-begin]"), header.index("[host-api-end]")
    for name in SYMBOLS:
        m = re.search(r"\b" + name + r"\b", header)
        assert m and begin < m.start() < end, name
    said = " ".join(header[begin:end].replace(" *", " ").split())
    # (the header's "c1 = *c": the comment's stars are taken out above)
    for text in ("c1 = c with jump_factor = 0", "resolves to 1 here, never to 10",
                 "S = 1 with jump_factor not > 0 is pikamd_cartesian_paths",
                 "S = 1 with jump_factor > 0 is pikamd_cartesian_paths when min_steps > 0 is given explicitly",
                 "1 here, 10 there", "relative to the tip pose of the state segment i-1 ended in",
                 "are the caller's max_joint_step, applied while walking", "S_p = 0 gives reached 0, steps 0, fraction 0",
                 "call again with W >= steps[p]", "approximate-solution gate is NOT applied", "S > W",
                 "KinematicsBase has none", "a grow frees"):
        assert text in said, text
    mirror = open(os.path.join(ROOT, "pick_ik_amd", "host", "pick_ik_amd.hpp")).read()
    assert "compute_cartesian_waypoints(" in mirror and "pikamd_cartesian_waypoints(" in mirror
    assert "struct CartesianWaypointsResult" in mirror and "segment_steps" in mirror
    shim = open(os.path.join(ROOT, "pick_ik_amd", "host", "pick_ik_plugin_shim.cpp")).read()
    assert "cartesian_waypoints" not in shim  # (KinematicsBase has no such entry)
    from pick_ik_amd import solver
    for strict in (False, True):
        L = solver.lib(strict)
        for name in SYMBOLS:
            assert name in solver.EXPORTED_SYMBOLS
            assert getattr(L, name).argtypes is not None, name
        assert len(L.pikamd_cartesian_waypoints.argtypes) == 19 and len(L.pikamd_cartesian_waypoints_device.argtypes) == 21
    for name in ("cartesian_waypoints", "cartesian_waypoints_device", "cartesian_waypoints_kernel_name"):
        assert callable(getattr(pk.Solver, name))
    assert C.sizeof(pk.Cartesian) == 32  # (reused unchanged)


def test_shape_checks_come_before_the_library(pk):
    """(no GPU here: a call that reached the library would fail for another reason)"""
    s = pk.Solver.__new__(pk.Solver)  # a handle-less object: the checks must raise before anything is called
    s.dof, s.n_tips, s._env_options = 7, 1, lambda: None
    p = pk.default_params(mode=1)
    c = pk.Cartesian(frame=2, max_translation=0.1)
    start, targets = np.zeros((4, 7)), np.zeros((4, 3, 7))
    with pytest.raises(ValueError, match="start"):
        s.cartesian_waypoints(p, c, np.zeros((4, 6)), targets, 5)
    with pytest.raises(ValueError, match="start"):
        s.cartesian_waypoints(p, c, np.zeros(7), targets, 5)
    with pytest.raises(ValueError, match="targets"):
        s.cartesian_waypoints(p, c, start, np.zeros((3, 3, 7)), 5)
    with pytest.raises(ValueError, match="targets"):
        s.cartesian_waypoints(p, c, start, np.zeros((4, 7)), 5)
    with pytest.raises(ValueError, match="targets"):
        s.cartesian_waypoints(p, c, start, np.zeros((4, 3, 6)), 5)
    with pytest.raises(ValueError, match="W >= S >= 1"):
        s.cartesian_waypoints(p, c, start, targets, 2)
    with pytest.raises(ValueError, match="W >= S >= 1"):
        s.cartesian_waypoints(p, c, start, np.zeros((4, 0, 7)), 5)
    with pytest.raises(ValueError, match="n_targets"):
        s.cartesian_waypoints(p, c, start, targets, 5, n_targets=np.zeros(3, dtype=np.int32))
    with pytest.raises(ValueError, match="max_joint_step"):
        s.cartesian_waypoints(p, c, start, targets, 5, max_joint_step=np.zeros(6))
    with pytest.raises(ValueError, match="W >= S >= 1"):
        s.cartesian_waypoints_device(p, c, 4, 3, 2, 1, 1, 1, 1, 1)
    with pytest.raises(ValueError, match="W >= S >= 1"):
        s.cartesian_waypoints_device(p, c, 4, 0, 2, 1, 1, 1, 1, 1)
    s._h = None


def kernel_names(fl, d):
    names = [f"polyline_segment_kernel<{d}>", f"polyline_finish_kernel<{d}>", f"ik_polyline_kernel<{d}>"]
    return names + ([f"ik_polyline_wide_kernel<{d},{l}>" for l in (16, 8)] if fl == "fast"
                    else [f"ik_polyline_team_kernel<{d},{l}>" for l in (16, 4)])


FLAVOURS = (("fast", "pik"), ("exact", "pik_exact"), ("strict", "pik_strict"))


def test_build_tables_name_the_family():
    from pick_ik_amd import build as Bd
    assert Bd.FAMILIES["pik_polyline_inst.hip"] == (("fast", "exact"), ("strict",))
    order = Bd.APPENDED_FAMILIES
    assert "pik_polyline_inst.hip" in order and order[-1] == "pik_globalpath_inst.hip"
    for strict, flavours in ((False, ("fast", "exact")), (True, ("strict",))):
        linked = Bd.link_objects(strict)
        objs = [o for o in linked if "pik_polyline" in o[0]]
        assert objs == [o for fl in flavours for o in Bd.family_objects("pik_polyline_inst.hip", fl)]
        assert linked[:len(Bd.library_objects(strict))] == Bd.library_objects(strict)
        # the memetic-start path objects are still the last
        last = [o for fl in flavours for o in Bd.family_objects("pik_globalpath_inst.hip", fl)]
        assert linked[-len(last):] == last
        assert not any("pik_cartesian" in o[0] for o in objs)


def test_committed_ledger_has_the_kernels():
    path = os.path.join(ROOT, "profiles", "r06_kernel_resources.csv")
    rows = {(r["flavour"], r["kernel"]): r for r in csv.DictReader(open(path))}
    n = [k for k in rows if "polyline" in k[1]]
    assert len(n) == 16 * (2 + 3) * 3
    assert {fl for fl, _ in n} == {"fast", "exact", "strict"}
    for fl, ns in FLAVOURS:
        for d in range(1, 17):
            for k in kernel_names(fl, d):
                assert (fl, f"{ns}::{k}") in rows, (fl, k)
    # no name is counted by the tests of the other families
    for _, k in n:
        for other in ("cartesian", "::ik_path", "::ik_search", "::ik_startpath", "::ik_globalpath", "::search_finalize",
                      "route_kernel", "restart_prepare", "restart_fold"):
            assert other not in k, (k, other)
    # a fast walk kernel spills no vector register and has no scratch, like its ik_cartesian_* twin
    for fl, k in n:
        if fl == "fast" and "::ik_polyline" in k:
            assert int(rows[(fl, k)]["vgpr_spills"]) == 0 and int(rows[(fl, k)]["scratch_bytes_per_lane"]) == 0, k
            twin = rows[(fl, k.replace("ik_polyline", "ik_cartesian"))]
            assert int(twin["vgpr_spills"]) == 0 and int(twin["scratch_bytes_per_lane"]) == 0, k


def test_the_kernels_are_reached_from_no_existing_translation_unit():
    from pick_ik_amd import build as Bd
    for tu in ("pik_inst.hip", "pik_path_inst.hip", "pik_search_inst.hip", "pik_route_inst.hip", "pik_restart_inst.hip",
               "pik_startpath_inst.hip", "pik_globalpath_inst.hip", "pik_cartesian_inst.hip", "pik_host_solve.hip"):
        for f in Bd._deps(tu, True):
            assert "pik_polyline" not in os.path.basename(f), (tu, f)
    ops = Bd._strip_comments(open(os.path.join(Bd.CSRC, "pik_polyline_ops.hpp")).read())
    assert not re.search(r"__global__|__device__|__shared__|__constant__", ops)
    seen = [os.path.basename(f) for f in Bd._deps("pik_amd.hip", True)]
    assert "pik_polyline_ops.hpp" in seen and "pik_polyline.hpp" not in seen
    # the kernels are built from the unchanged descents and the interpolation header
    seen = [os.path.basename(f) for f in Bd._deps("pik_polyline_inst.hip", True)]
    assert "pik_interp.hpp" in seen and "pik_path.hpp" in seen and "pik_cartesian.hpp" in seen


def test_a_hip_caller_compiles_against_the_header_and_the_mirror(tmp_path):
    """tests/native/polyline_api_check.hip calls the three entry points and Solver::compute_cartesian_waypoints from a
    .hip file: hipcc compiles it for gfx950, device pass included"""
    from pick_ik_amd import build as Bd
    src = os.path.join(ROOT, "tests", "native", "polyline_api_check.hip")
    r = subprocess.run([Bd.hipcc(), "--offload-arch=gfx950", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-c", src, "-o",
                        str(tmp_path / "polyline_api_check.o")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
