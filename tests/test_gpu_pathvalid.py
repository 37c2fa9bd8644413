"""The validity model inside the path entry points on the GPU (pikamd_set_path_validity): with the switch on and a
sphere model on the handle, pikamd_solve_paths, pikamd_cartesian_paths and pikamd_cartesian_waypoints end a path at the
first waypoint whose answer the model refuses.

Everything compares at tolerance zero, in every output array, with tests/pathvalid_reference.py: the loop with the step
`refused` over the CPU oracle for the exact builds, over the handle's own solve_batch + validity -- the definition --
for every flavour, the fast one included.  The fixtures are those of tests/test_pathvalid_cpu.py, which shows that the
oracle loops reach every class; the minima are asserted here again on what the GPU returns.  The edge shapes compare
with the post-pass form over the handle's own calls (the switch off, then the cut by hand), which the CPU tests hold to
the definition."""
import ctypes as C

import numpy as np
import pytest

import pick_ik_amd as pk
from pick_ik_amd import robots
from pick_ik_amd.solver import STATS_DTYPE
from tests import cartesian_reference as CR
from tests import path_reference as PR
from tests import pathvalid_reference as PV
from tests import polyline_reference as LR
from tests.hip_buffers import DeviceBuffers

pytestmark = pytest.mark.gpu
NO_PAIRS = np.zeros((0, 2), dtype=np.int32)
PATH_NAMES = ("solution", "status", "cost", "stats", "reached")
CART_NAMES = CR.NAMES + ("goals",)
LINE_NAMES = LR.NAMES
W_OFF = PV.W_OFFSETS
S_LINE, W_LINE = LR.S_POLYLINES, LR.W_POLYLINES
FLAVOURS = {"default_exact": dict(exact=None), "fast": dict(exact=False), "strict": dict(strict=True)}


@pytest.fixture(scope="module")
def O(oracle_mod):
    import __graft_entry__ as g
    g.build()
    return oracle_mod


def same(got, want, names, what=""):
    assert len(got) >= len(want), what
    for x, y, w in zip(got, want, names):
        np.testing.assert_array_equal(x, y, err_msg=f"{what}: {w}")


def own_valid(s):
    return lambda q: s.validity(q)[0]


def strict_of(s):
    return s._L is pk.solver.lib(True)


def lanes_of(s):
    return (1, 8, 16) if not (strict_of(s) or s.kernel_name(pk.default_params(mode=1)).startswith("pik_exact")) else (1, 4, 16)


# ---- pikamd_solve_paths -------------------------------------------------------------------------------
def test_solve_paths_equal_the_loop_over_the_oracle(O, exact_flavour):
    fx = PV.placed_paths(O, exact_flavour)
    s = pk.Solver(fx["chain"], device=0, strict=True)
    try:
        p = pk.default_params(mode=1)
        s.set_validity_model(*fx["model"])
        same(s.solve_paths(p, fx["goals"], fx["start"]), fx["plain"], PATH_NAMES, "switch off")
        s.set_path_validity(True)
        for lanes in (None, 1, 4, 16):
            s.set_option("lanes_per_elite", lanes)
            got = s.solve_paths(p, fx["goals"], fx["start"])
            same(got, fx["want"], PATH_NAMES, f"[{exact_flavour}] lanes {lanes}")
        cl = PV.cut_classes(fx["plain"][1], fx["plain"][4], got[1], got[4], PV.W_PATHS)
        print(f"placed obstacles [{exact_flavour}]: left alone / cut at row 0 / cut inside / distinct rows / cut on a "
              f"stopped path = {cl}")
        assert all(g >= m for g, m in zip(cl, PV.MINIMA_PATHS)), cl
        # sharding: the second half's paths alone give the second half
        h = PV.P_PATHS // 2
        same(s.solve_paths(p, fx["goals"][h:], fx["start"][h:]), [x[h:] for x in fx["want"]], PATH_NAMES, "second half")
        same(s.solve_paths(p, fx["goals"][:h], fx["start"][:h]), [x[:h] for x in fx["want"]], PATH_NAMES, "first half")
    finally:
        s.close()


@pytest.mark.parametrize("flavour", list(FLAVOURS))
def test_solve_paths_equal_the_loop_over_the_handles_own_calls(O, flavour):
    fx = PV.placed_paths(O, "fma")
    s = pk.Solver(fx["chain"], device=0, **FLAVOURS[flavour])
    try:
        step = np.full(7, 0.1)
        s.set_validity_model(*fx["model"])
        s.set_path_validity(True)
        for kw, lim in (({}, None), (dict(minimal_displacement_weight=0.001), step)):
            p = pk.default_params(mode=1, **kw)
            want = PV.reference_paths(lambda g, sd: s.solve_batch(p, g, sd), fx["goals"], fx["start"], lim, own_valid(s))
            assert (want[1] == PV.VALIDITY_REFUSED).any()  # (the comparison shows something: a path is cut)
            for lanes in lanes_of(s):
                s.set_option("lanes_per_elite", lanes)
                same(s.solve_paths(p, fx["goals"], fx["start"], lim), want, PATH_NAMES, f"{flavour} {kw} lanes {lanes}")
            s.set_option("lanes_per_elite", None)
    finally:
        s.close()


# ---- pikamd_cartesian_paths -----------------------------------------------------------------------------
@pytest.mark.parametrize("limit", [None, 0.1])
def test_cartesian_paths_equal_the_loop_over_the_oracle(O, exact_flavour, limit):
    from tests import validity_reference as V
    fx = PV.placed_offsets(O, pk, exact_flavour, limit)
    ch, start, target = fx["chain"], fx["start"], fx["target"]
    step = None if limit is None else np.full(ch.dof, limit)
    with O.math_mode(exact_flavour):
        o = O.Oracle(ch)
        po = O.default_params(mode=1)
        want0, _ = PV.reference_cartesian(lambda g, sd: o.solve_batch(po, g, sd, num_threads=O.max_threads()), fx["goals"],
                                          fx["steps"], start, 0.0, step, V.valid_of(V.oracle_fk_of(O, ch), fx["model"]))
    s = pk.Solver(ch, device=0, strict=True)
    try:
        p = pk.default_params(mode=1)
        c = pk.Cartesian(**CR.OFFSETS)
        c0 = pk.Cartesian(**dict(CR.OFFSETS, jump_factor=0.0, min_steps=3))
        s.set_validity_model(*fx["model"])
        same(s.cartesian_paths(p, c, start, target, W_OFF, step), fx["plain"] + (fx["goals"],), CART_NAMES, "switch off")
        s.set_path_validity(True)
        got = s.cartesian_paths(p, c, start, target, W_OFF, step)
        same(got, fx["want"] + (fx["goals"],), CART_NAMES, f"[{exact_flavour}] limit {limit}")
        # (the rows held before the relative test are the loop's: the arrays are its arrays)
        cl = PV.cartesian_classes(fx["plain"][1], fx["held_plain"], np.where(fx["steps"] <= W_OFF, fx["steps"], -1), got[1],
                                  fx["held"])
        print(f"placed offsets [{exact_flavour}] limit {limit}: {cl}")
        if limit is None:
            assert all(cl[k] >= m for k, m in PV.MINIMA_CARTESIAN.items()), cl
        assert cl["shown"] >= 4 and cl["alone"] >= 4, cl
        assert (got[5] > W_OFF).sum() >= 1  # (paths that were not walked: untouched, as the reference has them)
        same(s.cartesian_paths(p, c0, start, target, W_OFF, step), want0 + (fx["goals"],), CART_NAMES, "jump_factor 0")
        # the cut does not depend on an optional output
        lean = s.cartesian_paths(p, c, start, target, W_OFF, step, optional=False)
        for i in (0, 1, 5):
            np.testing.assert_array_equal(lean[i], fx["want"][i], err_msg=f"optional=False: {CART_NAMES[i]}")
        assert lean[2] is None and lean[4] is None and lean[6] is None
        h = len(start) // 2
        same(s.cartesian_paths(p, c, start[h:], target[h:], W_OFF, step), [x[h:] for x in fx["want"]], CART_NAMES, "second half")
    finally:
        s.close()


def handle_cartesian(s, p, c, start, target, w, step, valid_fn):
    goals, steps = pk.interpolate_poses(c, s.fk(start), target, w, strict=strict_of(s))
    out, _ = PV.reference_cartesian(lambda g, sd: s.solve_batch(p, g, sd), goals, steps, start, c.jump_factor, step, valid_fn)
    return out + (goals,)


@pytest.mark.parametrize("flavour", list(FLAVOURS))
def test_cartesian_paths_equal_the_loop_over_the_handles_own_calls(O, flavour):
    fx = PV.placed_offsets(O, pk, "fma")
    ch, start, target = fx["chain"], fx["start"], fx["target"]
    s = pk.Solver(ch, device=0, **FLAVOURS[flavour])
    try:
        s.set_validity_model(*fx["model"])
        s.set_path_validity(True)
        p = pk.default_params(mode=1)
        for jf, limit in ((CR.OFFSETS["jump_factor"], None), (0.0, 0.1), (CR.OFFSETS["jump_factor"], 0.1)):
            c = pk.Cartesian(**dict(CR.OFFSETS, jump_factor=jf))
            step = None if limit is None else np.full(ch.dof, limit)
            want = handle_cartesian(s, p, c, start, target, W_OFF, step, own_valid(s))
            assert (want[1] == PV.VALIDITY_REFUSED).any()  # (the comparison shows something: a path is cut)
            for lanes in lanes_of(s)[1:] + (None,):
                s.set_option("lanes_per_elite", lanes)
                same(s.cartesian_paths(p, c, start, target, W_OFF, step), want, CART_NAMES, f"{flavour} jf {jf} limit {limit} lanes {lanes}")
    finally:
        s.close()


# ---- pikamd_cartesian_waypoints ---------------------------------------------------------------------------
@pytest.mark.parametrize("limit", [None, 0.1])
def test_cartesian_waypoints_equal_the_loop_over_the_oracle(O, exact_flavour, limit):
    from tests import validity_reference as V
    fx = PV.placed_polylines(O, pk, exact_flavour, limit)
    ch, start, targets, nt = fx["chain"], fx["start"], fx["targets"], fx["n_targets"]
    step = None if limit is None else np.full(ch.dof, limit)
    c = pk.Cartesian(**LR.POLYLINES)
    c0 = pk.Cartesian(**dict(LR.POLYLINES, jump_factor=0.0))
    with O.math_mode(exact_flavour):
        o = O.Oracle(ch)
        po = O.default_params(mode=1)
        want0, _ = PV.reference_polyline(
            lambda g, sd: o.solve_batch(po, g, sd, num_threads=O.max_threads()), o.fk,
            lambda cc, a, t, w: pk.interpolate_poses(cc, a, t, w, strict=exact_flavour == "portable"), c0, start, targets,
            W_LINE, nt, step, V.valid_of(V.oracle_fk_of(O, ch), fx["model"]))
    s = pk.Solver(ch, device=0, strict=True)
    try:
        p = pk.default_params(mode=1)
        s.set_validity_model(*fx["model"])
        same(s.cartesian_waypoints(p, c, start, targets, W_LINE, nt, step), fx["plain"], LINE_NAMES, "switch off")
        s.set_path_validity(True)
        for lanes in (None, 1, 4, 16):
            s.set_option("lanes_per_elite", lanes)
            got = s.cartesian_waypoints(p, c, start, targets, W_LINE, nt, step)
            same(got, fx["want"], LINE_NAMES, f"[{exact_flavour}] limit {limit} lanes {lanes}")
        s.set_option("lanes_per_elite", None)
        ip = fx["info_plain"]
        cl = PV.cartesian_classes(fx["plain"][1], ip["held"], np.where(ip["kind"] == LR.COMPLETE, ip["held"], -1), got[1],
                                  fx["info"]["held"])
        later = PV.cut_behind_the_first_segment(ip["held"], fx["info"]["held"], got[8], fx["info"]["seg"])
        print(f"placed polylines [{exact_flavour}] limit {limit}: {cl}, cut behind segment 0: {later}")
        assert all(cl[k] >= m for k, m in PV.MINIMA_CARTESIAN.items()) and later >= 2, (cl, later)
        same(s.cartesian_waypoints(p, c0, start, targets, W_LINE, nt, step), want0, LINE_NAMES, "jump_factor 0")
        lean = s.cartesian_waypoints(p, c, start, targets, W_LINE, nt, step, optional=False)
        for i in (0, 1, 5):
            np.testing.assert_array_equal(lean[i], fx["want"][i], err_msg=f"optional=False: {LINE_NAMES[i]}")
        assert lean[2] is None and lean[4] is None and lean[8] is None
        h = len(start) // 2
        same(s.cartesian_waypoints(p, c, start[h:], targets[h:], W_LINE, nt[h:], step), [x[h:] for x in fx["want"]],
             LINE_NAMES, "second half")
    finally:
        s.close()


@pytest.mark.parametrize("flavour", list(FLAVOURS))
def test_cartesian_waypoints_equal_the_loop_over_the_handles_own_calls(O, flavour):
    fx = PV.placed_polylines(O, pk, "fma")
    ch, start, targets, nt = fx["chain"], fx["start"], fx["targets"], fx["n_targets"]
    s = pk.Solver(ch, device=0, **FLAVOURS[flavour])
    try:
        s.set_validity_model(*fx["model"])
        s.set_path_validity(True)
        p = pk.default_params(mode=1)
        for jf, limit in ((LR.POLYLINES["jump_factor"], None), (0.0, 0.1)):
            c = pk.Cartesian(**dict(LR.POLYLINES, jump_factor=jf))
            step = None if limit is None else np.full(ch.dof, limit)
            want, _ = PV.reference_polyline(lambda g, sd: s.solve_batch(p, g, sd), s.fk,
                                            lambda cc, a, t, w: pk.interpolate_poses(cc, a, t, w, strict=strict_of(s)), c,
                                            start, targets, W_LINE, nt, step, own_valid(s))
            assert (want[1] == PV.VALIDITY_REFUSED).any()  # (the comparison shows something: a path is cut)
            same(s.cartesian_waypoints(p, c, start, targets, W_LINE, nt, step), want, LINE_NAMES, f"{flavour} jf {jf} limit {limit}")
    finally:
        s.close()


# ---- the switch off, no model, the entry points out of scope -------------------------------------------------
def _three_calls(s, p, fx_p, fx_o, fx_l):
    c, cl = pk.Cartesian(**CR.OFFSETS), pk.Cartesian(**LR.POLYLINES)
    return (s.solve_paths(p, fx_p["goals"][:16], fx_p["start"][:16]),
            s.cartesian_paths(p, c, fx_o["start"], fx_o["target"], W_OFF),
            s.cartesian_waypoints(p, cl, fx_l["start"], fx_l["targets"], W_LINE, fx_l["n_targets"]))


@pytest.mark.parametrize("flavour", ["default_exact", "fast"])
def test_switch_off_or_no_model_changes_nothing(O, flavour):
    fx_p, fx_o, fx_l = PV.placed_paths(O, "fma"), PV.placed_offsets(O, pk, "fma"), PV.placed_polylines(O, pk, "fma")
    p = pk.default_params(mode=1)
    s = pk.Solver(fx_p["chain"], device=0, **FLAVOURS[flavour])
    try:
        never = _three_calls(s, p, fx_p, fx_o, fx_l)
        s.set_path_validity(True)  # on, no model
        for got, want, names in zip(_three_calls(s, p, fx_p, fx_o, fx_l), never, (PATH_NAMES, CART_NAMES, LINE_NAMES)):
            same(got, want, names, "on, no model")
        s.set_validity_model(*fx_p["model"])
        assert (s.solve_paths(p, fx_p["goals"][:16], fx_p["start"][:16])[1] == PV.VALIDITY_REFUSED).any()
        s.set_path_validity(False)  # off, a model
        for got, want, names in zip(_three_calls(s, p, fx_p, fx_o, fx_l), never, (PATH_NAMES, CART_NAMES, LINE_NAMES)):
            same(got, want, names, "off, a model")
        s.set_path_validity(True)
        s.clear_validity_model()  # (the switch stays on: nothing to apply)
        for got, want, names in zip(_three_calls(s, p, fx_p, fx_o, fx_l), never, (PATH_NAMES, CART_NAMES, LINE_NAMES)):
            same(got, want, names, "model cleared")
        with pytest.raises(pk.PickIkAmdError, match="expected 0 or 1"):
            s._chk(s._L.pikamd_set_path_validity(s._h, 2))
    finally:
        s.close()


def test_the_search_path_entry_points_keep_ignoring_the_model(O):
    fx = PV.placed_paths(O, "fma")
    goals, start = fx["goals"][:24, :8], fx["start"][:24]
    s = pk.Solver(fx["chain"], device=0)
    try:
        s.set_validity_model(*fx["model"])
        pl = pk.default_params(mode=1)
        pg = pk.default_params(mode=0, memetic_population_size=16, memetic_max_generations=6)
        off = (s.search_paths(pl, goals, start, 3, rng_seed=5), s.search_global_paths(pg, goals, start, 2, rng_seed=5))
        s.set_path_validity(True)
        on = (s.search_paths(pl, goals, start, 3, rng_seed=5), s.search_global_paths(pg, goals, start, 2, rng_seed=5))
        for a, b in zip(off, on):
            for x, y in zip(a, b):
                np.testing.assert_array_equal(x, y)
            assert not (b[1] == PV.VALIDITY_REFUSED).any()
    finally:
        s.close()


# ---- edge shapes ----------------------------------------------------------------------------------------------
def cut_by_hand(s, p, goals, start, step=None):
    """the post-pass over the handle's own calls: the walk with the switch off, then the cut"""
    s.set_path_validity(False)
    plain = s.solve_paths(p, goals, start, step)
    s.set_path_validity(True)
    return plain, PV.cut_paths(plain, start, own_valid(s))


@pytest.mark.parametrize("flavour", ["default_exact", "strict"])
@pytest.mark.parametrize("P,W,rows", [(3, 1, (0,)), (3, 2, (1, 0)), (3, 33, (32, 5, 0)), (3, 70, (69, 64, 33)), (1, 16, (9,)),
                                      (65, 16, (15, 0, 7))])
def test_edge_shapes(O, flavour, P, W, rows):
    """W = 1, 2; W = 33 and 70: more rows than one round of the team; P = 1; P = 65: a second block.  A needle model
    -- one sphere of 1 mm on the hand against obstacles of 1 mm where the hand of path i is at rows[i], so that a path
    is cut AT that row and not a hand's width in front of it -- the last row of a complete path, row 0 (the held state
    is the start), a row of the second round among them"""
    ch = robots.panda()
    s = pk.Solver(ch, device=0, **FLAVOURS[flavour])
    try:
        p = pk.default_params(mode=1)
        goals, start = PR.joint_lines(ch, s.fk, P=P, W=W)
        plain = s.solve_paths(p, goals, start)
        needle = [(6, (0.0, 0.0, 0.14), 0.001)]
        s.set_validity_model(needle, NO_PAIRS)
        centres = [s.validity(plain[0][i, k][None], centres=True)[2][0, 0] for i, k in enumerate(rows[:P])]
        obstacles = [(-1, tuple(float(v) for v in c), 0.001) for c in centres]
        s.set_validity_model(needle + obstacles, np.array([(0, 1 + i) for i in range(len(obstacles))], dtype=np.int32))
        plain2, want = cut_by_hand(s, p, goals, start)
        same(plain2, plain, PATH_NAMES, "switch off")
        got = s.solve_paths(p, goals, start)
        same(got, want, PATH_NAMES, f"{flavour} P {P} W {W}")
        refused = got[1] == PV.VALIDITY_REFUSED
        at = np.where(refused.any(axis=1), np.argmax(refused, axis=1), -1)
        print(f"edge P {P} W {W}: plain reached {plain[4][:3].tolist()}, cut rows {at[:3].tolist()}")
        assert (at >= 0).any(), "no path was cut"
        for i, k in enumerate(rows[:P]):
            if plain[4][i] > k:  # the plain walk held the obstacle's row: the path is cut there, or in front of it
                assert 0 <= at[i] <= k, (i, k, at[i])
        if (P, W) == (3, 70) and plain[4][0] == 70:
            assert at.max() >= 64  # (a refusal found in the second round of 64 rows)
    finally:
        s.close()


def test_model_without_a_pair_and_model_at_the_cap(O):
    fx = PV.placed_paths(O, "fma")
    goals, start = fx["goals"], fx["start"]
    s = pk.Solver(fx["chain"], device=0)
    try:
        p = pk.default_params(mode=1)
        plain = s.solve_paths(p, goals, start)
        s.set_path_validity(True)
        s.set_validity_model([(6, (0.0, 0.0, 0.14), 0.07)], np.zeros((0, 2), dtype=np.int32))
        same(s.solve_paths(p, goals, start), plain, PATH_NAMES, "one sphere, no pair")
        # PIKAMD_MAX_SPHERES spheres and PIKAMD_MAX_SPHERE_PAIRS pairs: 48 KiB of LDS per block
        spheres, pairs = fx["model"]
        far = [(-1, (5.0 + 0.1 * i, 5.0, 5.0), 0.01) for i in range(pk.solver.MAX_SPHERES - len(spheres))]
        spheres = list(spheres) + far
        first = len(spheres) - len(far)
        extra = [(i, j) for j in range(first, 32) for i in range(9)] + [(i, j) for i in range(first, 32) for j in range(i + 1, 32)]
        pairs = np.concatenate([pairs, np.array(extra, dtype=np.int32)])[:pk.solver.MAX_SPHERE_PAIRS]
        assert len(spheres) == 32 and len(pairs) == 256
        s.set_validity_model(spheres, pairs)
        _, want = cut_by_hand(s, p, goals, start)
        assert (want[1] == PV.VALIDITY_REFUSED).any(axis=1).sum() >= 8
        same(s.solve_paths(p, goals, start), want, PATH_NAMES, "model at the cap")
    finally:
        s.close()


def test_scratch_grows_and_shrinks_on_one_slot(O):
    """calls with reached = NULL (its count lives in the slot's scratch): a smaller and then a larger call on the same
    handle give what a fresh handle gives"""
    fx = PV.placed_offsets(O, pk, "fma")
    ch, start, target = fx["chain"], fx["start"], fx["target"]
    p = pk.default_params(mode=1)
    c = pk.Cartesian(**CR.OFFSETS)
    shapes = ((20, 12), (5, 6), (70, 16))
    s = pk.Solver(ch, device=0)
    try:
        s.set_validity_model(*fx["model"])
        s.set_path_validity(True)
        got = [s.cartesian_paths(p, c, start[:n], target[:n], w, optional=False) for n, w in shapes]
    finally:
        s.close()
    for (n, w), g in zip(shapes, got):
        f = pk.Solver(ch, device=0)
        try:
            f.set_validity_model(*fx["model"])
            f.set_path_validity(True)
            want = f.cartesian_paths(p, c, start[:n], target[:n], w)
        finally:
            f.close()
        for i in (0, 1, 5):
            np.testing.assert_array_equal(g[i], want[i], err_msg=f"P {n} W {w}: {CART_NAMES[i]}")
        assert w != 12 or (want[1] == PV.VALIDITY_REFUSED).any()


# ---- the _device forms on a caller's stream ------------------------------------------------------------------
def test_device_forms_give_the_host_forms_arrays(O):
    fx_p, fx_o, fx_l = PV.placed_paths(O, "fma"), PV.placed_offsets(O, pk, "fma"), PV.placed_polylines(O, pk, "fma")
    ch = fx_p["chain"]
    p = pk.default_params(mode=1)
    s = pk.Solver(ch, device=0)
    d = DeviceBuffers()
    stream = C.c_void_p()
    try:
        s.set_validity_model(*fx_p["model"])
        s.set_path_validity(True)
        d.hip.hipStreamCreate.argtypes = [C.POINTER(C.c_void_p)]
        d.hip.hipStreamSynchronize.argtypes = [C.c_void_p]
        d.hip.hipStreamDestroy.argtypes = [C.c_void_p]
        assert d.hip.hipStreamCreate(C.byref(stream)) == 0
        # solve_paths: with every output, and with reached left out
        goals, start = fx_p["goals"], fx_p["start"]
        P, W = goals.shape[:2]
        want = s.solve_paths(p, goals, start)
        for with_optional in (True, False):
            sol, st = d.alloc(8 * P * W * 7), d.alloc(4 * P * W)
            cost, stats, reached = (d.alloc(8 * P * W), d.alloc(STATS_DTYPE.itemsize * P * W), d.alloc(4 * P)) if with_optional else (0, 0, 0)
            s.solve_paths_device(p, P, W, d.upload(goals), d.upload(start), sol, st, 0, cost, stats, reached,
                                 stream=stream.value, slot=1)
            assert d.hip.hipStreamSynchronize(stream) == 0
            np.testing.assert_array_equal(d.download(sol, (P, W, 7), np.float64), want[0])
            np.testing.assert_array_equal(d.download(st, (P, W), np.int32), want[1])
            if with_optional:
                np.testing.assert_array_equal(d.download(cost, (P, W), np.float64), want[2])
                np.testing.assert_array_equal(d.download(stats, (P, W), STATS_DTYPE), want[3])
                np.testing.assert_array_equal(d.download(reached, (P,), np.int32), want[4])
        # cartesian_paths: reached, fraction and goals left out
        s.set_validity_model(*fx_o["model"])
        c = pk.Cartesian(**CR.OFFSETS)
        start, target = fx_o["start"], fx_o["target"]
        P, W = len(start), W_OFF
        want = s.cartesian_paths(p, c, start, target, W)
        for with_optional in (True, False):
            sol, st, steps = d.alloc(8 * P * W * 7), d.alloc(4 * P * W), d.alloc(4 * P)
            reached, fraction = (d.alloc(4 * P), d.alloc(8 * P)) if with_optional else (0, 0)
            s.cartesian_paths_device(p, c, P, W, d.upload(start), d.upload(target), sol, st, steps, d_reached=reached,
                                     d_fraction=fraction, stream=stream.value, slot=2)
            assert d.hip.hipStreamSynchronize(stream) == 0
            np.testing.assert_array_equal(d.download(sol, (P, W, 7), np.float64), want[0])
            np.testing.assert_array_equal(d.download(st, (P, W), np.int32), want[1])
            np.testing.assert_array_equal(d.download(steps, (P,), np.int32), want[5])
            if with_optional:
                np.testing.assert_array_equal(d.download(reached, (P,), np.int32), want[4])
                np.testing.assert_array_equal(d.download(fraction, (P,), np.float64), want[6])
        # cartesian_waypoints
        s.set_validity_model(*fx_l["model"])
        cl = pk.Cartesian(**LR.POLYLINES)
        start, targets, nt = fx_l["start"], fx_l["targets"], fx_l["n_targets"]
        P, W = len(start), W_LINE
        want = s.cartesian_waypoints(p, cl, start, targets, W, nt)
        sol, st, steps, reached, fraction = d.alloc(8 * P * W * 7), d.alloc(4 * P * W), d.alloc(4 * P), d.alloc(4 * P), d.alloc(8 * P)
        s.cartesian_waypoints_device(p, cl, P, S_LINE, W, d.upload(start), d.upload(targets), sol, st, steps,
                                     d_n_targets=d.upload(nt), d_reached=reached, d_fraction=fraction, stream=stream.value, slot=3)
        assert d.hip.hipStreamSynchronize(stream) == 0
        np.testing.assert_array_equal(d.download(sol, (P, W, 7), np.float64), want[0])
        np.testing.assert_array_equal(d.download(st, (P, W), np.int32), want[1])
        np.testing.assert_array_equal(d.download(reached, (P,), np.int32), want[4])
        np.testing.assert_array_equal(d.download(steps, (P,), np.int32), want[5])
        np.testing.assert_array_equal(d.download(fraction, (P,), np.float64), want[6])
        assert (want[1] == PV.VALIDITY_REFUSED).any()
    finally:
        d.free()
        if stream.value:
            d.hip.hipStreamDestroy(stream)
        s.close()


# ---- every optional output NULL in turn: the cut does not depend on one ------------------------------------------
def test_cartesian_paths_without_each_optional_array(O):
    from tests import test_gpu_cartesian as TC
    fx = PV.placed_offsets(O, pk, "fma")
    n = 9  # (odd: the int32 arrays end off an 8-byte boundary; the first obstacles sit on these paths)
    start, target = fx["start"][:n], fx["target"][:n]
    s = pk.Solver(fx["chain"], device=0)
    try:
        s.set_validity_model(*fx["model"])
        s.set_path_validity(True)
        p, c = pk.default_params(mode=1), pk.Cartesian(**CR.OFFSETS)
        full = TC._pattern(n, 7)
        assert TC._raw(s, p, c, start, target, None, full) == 0
        same([full[k] for k in TC.ORDER], [x[:n] for x in fx["want"]] + [fx["goals"][:n]], CART_NAMES, "every array")
        assert (full["status"] == PV.VALIDITY_REFUSED).any(axis=1).sum() >= 3
        for gone in ("final_cost", "stats", "reached", "fraction", "goals"):
            a = TC._pattern(n, 7)
            a[gone] = None
            assert TC._raw(s, p, c, start, target, None, a) == 0, gone
            for k in TC.ORDER:
                if a[k] is not None:
                    assert a[k].tobytes() == full[k].tobytes(), f"without {gone}: {k} differs"
    finally:
        s.close()


def test_cartesian_waypoints_without_each_optional_array(O):
    from tests import test_gpu_polyline as TL
    fx = PV.placed_polylines(O, pk, "fma")
    n = 35  # (odd; the first obstacles sit on paths 18 .. 25)
    start, targets, nt = fx["start"][:n], fx["targets"][:n], fx["n_targets"][:n]
    s = pk.Solver(fx["chain"], device=0)
    try:
        s.set_validity_model(*fx["model"])
        s.set_path_validity(True)
        p, c = pk.default_params(mode=1), pk.Cartesian(**LR.POLYLINES)
        full = TL._pattern(n, 7)
        assert TL._raw(s, p, c, start, targets, nt, None, full) == 0
        same([full[k] for k in TL.ORDER], [x[:n] for x in fx["want"]], LINE_NAMES, "every array")
        assert (full["status"] == PV.VALIDITY_REFUSED).any(axis=1).sum() >= 3
        for gone in ("final_cost", "stats", "reached", "fraction", "goals", "segment_steps"):
            a = TL._pattern(n, 7)
            a[gone] = None
            assert TL._raw(s, p, c, start, targets, nt, None, a) == 0, gone
            for k in TL.ORDER:
                if a[k] is not None:
                    assert a[k].tobytes() == full[k].tobytes(), f"without {gone}: {k} differs"
    finally:
        s.close()
