"""computeCartesianPath in one call (CPU): pikamd_interpolate_poses of both libraries against a 50-digit restatement
of its definition, the normative loop of pikamd_cartesian_paths (tests/cartesian_reference.py) over the CPU oracle on
the fixtures of the GPU tests -- each must reach every class, so that the GPU comparison (tests/test_gpu_cartesian.py)
cannot pass on one branch only --, the shape of the rows behind every kind of stop, the declarations, the shape checks,
the resource ledger of the new kernels and a sanitizer run of the interpolation header."""
import csv
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from tests import cartesian_reference as CR
from tests import path_reference as PR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("pikamd_interpolate_poses", "pikamd_cartesian_paths", "pikamd_cartesian_paths_device",
           "pikamd_cartesian_kernel_name")
W_OFFSETS = 12

#: Interpolation accuracy: the worst error measured over the generated cases of test_interpolation_accuracy, both
#: libraries (DESIGN.md section 3 records them) -- positions relative to max(|ta|, |tb|, 1), quaternion components
#: absolute.  The test asserts 4 times the measured figure; the issue caps the asserted bound at 1e-13.
MEASURED_POSITION = 2.0e-16
MEASURED_QUATERNION = 3.9e-16


@pytest.fixture(params=["portable", "fma"])
def mode(request):
    return request.param


@pytest.fixture(scope="module")
def pk():
    import __graft_entry__ as g
    g.build()
    import pick_ik_amd
    return pick_ik_amd


# ---- interpolation accuracy -----------------------------------------------------------------------
def _unit(rng, n):
    q = rng.normal(size=(n, 4))
    return q / np.linalg.norm(q, axis=1, keepdims=True)


def _about(rng, q, angle):
    """q times a rotation of `angle` [n] about random axes (Hamilton product, rounded: the inputs are what they are)"""
    ax = rng.normal(size=(len(q), 3))
    ax /= np.linalg.norm(ax, axis=1, keepdims=True)
    r = np.concatenate([np.cos(0.5 * angle)[:, None], np.sin(0.5 * angle)[:, None] * ax], axis=1)
    return CR._quat_mul(q, r)


def pose_pairs(frame, n=2000, seed=3):
    """start poses and targets of one frame mode: translations up to 0.5, rotations up to pi, and the edge cases -- a
    rotation of 0, rotations within 1e-9 of 0, within 1e-6 of pi, the target quaternion negated (d < 0), start and
    target equal"""
    rng = np.random.default_rng(seed + frame)
    a = np.concatenate([rng.uniform(-1.0, 1.0, size=(n, 3)), _unit(rng, n)], axis=1)
    angle = rng.uniform(0.0, np.pi, size=n)
    angle[0:40] = 0.0
    angle[40:80] = rng.uniform(0.0, 1e-9, size=40)
    angle[80:120] = np.pi - rng.uniform(0.0, 1e-6, size=40)
    shift = rng.normal(size=(n, 3))
    shift *= rng.uniform(0.0, 0.5, size=(n, 1)) / np.linalg.norm(shift, axis=1, keepdims=True)
    if frame == 1:  # relative to the tip: a rotation and a shift in the tip frame
        t = np.concatenate([shift, _about(rng, np.tile([1.0, 0.0, 0.0, 0.0], (n, 1)), angle)], axis=1)
        t[0:40, 3:] = [1.0, 0.0, 0.0, 0.0]
        t[160:200, :3] = 0.0  # start and target equal
        t[160:200, 3:] = [1.0, 0.0, 0.0, 0.0]
    else:
        t = np.concatenate([a[:, :3] + shift, _about(rng, a[:, 3:], angle)], axis=1)
        t[0:40, 3:] = a[0:40, 3:]
        t[160:200] = a[160:200]
        if frame == 2:
            t[:, :3] = shift
            t[160:200, :3] = 0.0
    t[120:160, 3:] *= -1.0  # d < 0 (frames 0 and 1; the offset frame ignores the quaternion)
    return a, t


def mp_interpolate(frame, min_steps, max_t, max_r, W, a, t, n_given=None):
    """the definition of pikamd_interpolate_poses in 50 digits, one path: (rows [W][7] of mpf, n, sure); sure is False
    when a step quotient lies within 1e-9 of an integer above 0 (a quotient is never negative, so the floor of one
    near 0 is 0 either way): the floor could go either way, and n_given then says which way the rows are to go"""
    import mpmath as mp
    f = lambda v: [mp.mpf(float(x)) for x in v]
    ta, qa, tt, qt = f(a[:3]), f(a[3:]), f(t[:3]), f(t[3:])

    def mul(p, q):
        return [p[0] * q[0] - p[1] * q[1] - p[2] * q[2] - p[3] * q[3], p[0] * q[1] + p[1] * q[0] + p[2] * q[3] - p[3] * q[2],
                p[0] * q[2] - p[1] * q[3] + p[2] * q[0] + p[3] * q[1], p[0] * q[3] + p[1] * q[2] - p[2] * q[1] + p[3] * q[0]]

    if frame == 0:
        tb, qb = tt, qt
    elif frame == 1:
        w, x, y, z = qa  # Eigen's toRotationMatrix, no normalisation
        R = [[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
             [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
             [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]]
        tb = [ta[i] + sum(R[i][j] * tt[j] for j in range(3)) for i in range(3)]
        qb = mul(qa, qt)
    else:
        tb, qb = [ta[i] + tt[i] for i in range(3)], qa
    trans = mp.sqrt(sum((tb[i] - ta[i]) ** 2 for i in range(3)))
    d = mul(qa, [qb[0], -qb[1], -qb[2], -qb[3]])
    rot = 2 * mp.atan2(mp.sqrt(d[1] ** 2 + d[2] ** 2 + d[3] ** 2), abs(d[0]))
    sure, most = True, 0
    for dist, lim in ((trans, max_t), (rot, max_r)):
        if lim > 0:
            q = dist / mp.mpf(lim)
            near = mp.nint(q)
            if near >= 1 and abs(q - near) < mp.mpf("1e-9"):
                sure = False
            most = max(most, int(mp.floor(q)))
    n = max(most + 1, min_steps) if n_given is None else n_given
    b = tb + qb
    if n > W:
        return [b] * W, n, sure
    dot = sum(qa[i] * qb[i] for i in range(4))
    rows = []
    for k in range(W):
        if k >= n:
            rows.append(b)
            continue
        pct = mp.mpf(k + 1) / n
        if abs(dot) >= 1 - mp.mpf(2) ** -52:
            s0, s1 = 1 - pct, pct
        else:
            th = mp.acos(abs(dot))
            s0, s1 = mp.sin((1 - pct) * th) / mp.sin(th), mp.sin(pct * th) / mp.sin(th)
        if dot < 0:
            s1 = -s1
        rows.append([pct * tb[i] + (1 - pct) * ta[i] for i in range(3)] + [s0 * qa[i] + s1 * qb[i] for i in range(4)])
    return rows, n, sure


@pytest.mark.parametrize("strict", [False, True], ids=["product", "verification"])
def test_interpolation_accuracy(pk, strict):
    import mpmath as mp
    mp.mp.dps = 50
    W, max_t, max_r = 8, 0.1, 0.5
    worst_p, worst_q, left_out, total = 0.0, 0.0, 0, 0
    for frame in (0, 1, 2):
        a, t = pose_pairs(frame)
        c = pk.Cartesian(frame=frame, min_steps=2, max_translation=max_t, max_rotation=max_r)
        goals, steps = pk.interpolate_poses(c, a, t, W, strict=strict)
        for p in range(len(a)):
            rows, n, sure = mp_interpolate(frame, 2, max_t, max_r, W, a[p], t[p])
            total += 1
            if sure:
                assert steps[p] == n, (frame, p, steps[p], n)
            else:  # left out of the step comparison, not of the pose comparison: the poses of the library's count
                left_out += 1
                assert abs(int(steps[p]) - n) <= 1, (frame, p, steps[p], n)
                if steps[p] != n:
                    rows, n, _ = mp_interpolate(frame, 2, max_t, max_r, W, a[p], t[p], n_given=int(steps[p]))
            assert n <= W  # (the generator keeps every path inside W: the waypoints are compared, not the target only)
            tb = [float(x) for x in rows[W - 1][:3]]
            scale = max(np.linalg.norm(a[p, :3]), np.linalg.norm(tb), 1.0)
            for k in range(W):
                for i in range(7):
                    e = abs(float(mp.mpf(float(goals[p, k, i])) - rows[k][i]))
                    if i < 3:
                        worst_p = max(worst_p, e / scale)
                    else:
                        worst_q = max(worst_q, e)
    print(f"interpolate_poses [{'verification' if strict else 'product'}]: worst position error {worst_p:.3g} (relative), "
          f"worst quaternion error {worst_q:.3g}; {left_out} of {total} step counts left out")
    assert left_out < 0.01 * total
    assert 4 * MEASURED_POSITION <= 1e-13 and 4 * MEASURED_QUATERNION <= 1e-13
    assert worst_p <= 4 * MEASURED_POSITION, worst_p
    assert worst_q <= 4 * MEASURED_QUATERNION, worst_q


def test_interpolation_edges_and_refusals(pk):
    """no device: the step rule, the rows behind the steps, a path longer than W, and every refusal"""
    a = np.array([[0.1, 0.2, 0.3, 1.0, 0.0, 0.0, 0.0]])
    t = np.array([[0.255, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0]])
    b = [a[0, 0] + t[0, 0], 0.2, 0.3, 1.0, 0.0, 0.0, 0.0]
    for strict in (False, True):
        goals, steps = pk.interpolate_poses(pk.Cartesian(frame=2, max_translation=0.1), a, t, 5, strict=strict)
        assert steps[0] == 3  # floor(0.255 / 0.1) + 1
        np.testing.assert_array_equal(goals[0, 2], b)  # the last waypoint is the target
        np.testing.assert_array_equal(goals[0, 3:], np.tile(goals[0, 2], (2, 1)))
        assert abs(goals[0, 0, 0] - (0.1 + 0.255 / 3)) < 1e-15
        # MoveIt's minimum: 10 with a relative test, 1 without; a given one as it is
        assert pk.interpolate_poses(pk.Cartesian(frame=2, max_translation=1.0, jump_factor=2.0), a, t, 12, strict=strict)[1][0] == 10
        assert pk.interpolate_poses(pk.Cartesian(frame=2, max_translation=1.0), a, t, 12, strict=strict)[1][0] == 1
        assert pk.interpolate_poses(pk.Cartesian(frame=2, max_translation=1.0, min_steps=4, jump_factor=2.0), a, t, 12, strict=strict)[1][0] == 4
        # longer than W: the count, and every row the target
        goals, steps = pk.interpolate_poses(pk.Cartesian(frame=2, max_translation=0.01), a, t, 5, strict=strict)
        assert steps[0] == 26
        np.testing.assert_array_equal(goals[0], np.tile(b, (5, 1)))
        # a quotient that is not finite, or not below 2^31
        assert pk.interpolate_poses(pk.Cartesian(frame=2, max_translation=1e-12), a, t, 5, strict=strict)[1][0] == 2**31 - 1
        bad = t.copy()
        bad[0, 0] = np.nan
        assert pk.interpolate_poses(pk.Cartesian(frame=2, max_translation=0.1), a, bad, 5, strict=strict)[1][0] == 2**31 - 1
        # a rotation by pi about z in the tip frame, half a step each: slerp goes through the quarter turn
        turn = np.array([[0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 1.0]])
        goals, steps = pk.interpolate_poses(pk.Cartesian(frame=1, max_rotation=2.0), a, turn, 2, strict=strict)
        assert steps[0] == 2
        np.testing.assert_allclose(goals[0, 0, 3:], [np.sqrt(0.5), 0.0, 0.0, np.sqrt(0.5)], atol=1e-15)
        np.testing.assert_array_equal(goals[0, 1, 3:], [0.0, 0.0, 0.0, 1.0])
        # no path: nothing to do
        g0, s0 = pk.interpolate_poses(pk.Cartesian(frame=0, max_translation=0.1), np.zeros((0, 7)), np.zeros((0, 7)), 3, strict=strict)
        assert g0.shape == (0, 3, 7) and s0.shape == (0,)
        # refusals: PIKAMD_EINVAL (-1) and a message, without a device
        L = pk.solver.lib(strict)
        dp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int32)
        g, st = np.empty((1, 5, 7)), np.empty(1, dtype=np.int32)
        ok = pk.Cartesian(frame=0, max_translation=0.1)

        def raw(c=ok, W=5, start=a, target=t, goals_=g, steps_=st):
            ptr = lambda x, ty: None if x is None else x.ctypes.data_as(ty)
            return L.pikamd_interpolate_poses(None if c is None else C.byref(c), 1, W, ptr(start, dp), ptr(target, dp),
                                              ptr(goals_, dp), ptr(steps_, ip))

        assert raw() == 0
        assert raw(c=None) == -1
        for name in ("start", "target", "goals_", "steps_"):
            assert raw(**{name: None}) == -1 and "must not be NULL" in L.pikamd_last_error().decode(), name
        assert raw(c=pk.Cartesian(frame=3, max_translation=0.1)) == -1 and "frame" in L.pikamd_last_error().decode()
        assert raw(c=pk.Cartesian(frame=-1, max_translation=0.1)) == -1
        assert raw(W=0) == -1 and "W >= 1" in L.pikamd_last_error().decode()
        assert raw(c=pk.Cartesian(frame=0, max_translation=0.1, min_steps=-1)) == -1 and "min_steps" in L.pikamd_last_error().decode()
        assert raw(c=pk.Cartesian(frame=0)) == -1 and "neither" in L.pikamd_last_error().decode()
        assert raw(c=pk.Cartesian(frame=0, max_translation=float("nan"), max_rotation=-1.0)) == -1


# ---- the normative loop over the oracle -------------------------------------------------------------
def oracle_offsets(O, pk, limit, strict):
    """the fixture "panda offsets" through the loop over the oracle, in the math mode set; strict: the library whose
    host interpolation makes the poses (the verification library under "portable", the product library under "fma")"""
    ch = pk.robots.panda()
    o = O.Oracle(ch)
    start, target = CR.offsets(ch)
    goals, steps = pk.interpolate_poses(pk.Cartesian(**CR.OFFSETS), o.fk(start), target, W_OFFSETS, strict=strict)
    po = O.default_params(mode=1)
    step = None if limit is None else np.full(ch.dof, limit)
    out, held = CR.reference_cartesian(lambda g, sd: o.solve_batch(po, g, sd, num_threads=O.max_threads()), goals, steps,
                                       start, CR.OFFSETS["jump_factor"], step)
    return ch, start, goals, out, held


def test_fixture_reaches_every_class(oracle_mod, pk, mode):
    O = oracle_mod
    with O.math_mode(mode):
        _, _, _, free, held_free = oracle_offsets(O, pk, None, mode == "portable")
        _, _, _, lim, held_lim = oracle_offsets(O, pk, 0.1, mode == "portable")
    cf, cl = CR.classes(free, held_free, W_OFFSETS), CR.classes(lim, held_lim, W_OFFSETS)
    names = "complete / solver / absolute / relative / too long / relative on a complete path"
    print(f"panda offsets [{mode}] steps {free[5].min()}..{free[5].max()}: no limit {cf}, limit 0.1 {cl} ({names})")
    complete, solver, absolute, relative, long_, on_complete = cf
    assert min(complete, solver, relative, long_) >= 4 and absolute == 0 and on_complete >= 1, cf
    assert min(cl[:5]) >= 4, cl
    assert len(set(free[5][free[5] <= W_OFFSETS])) >= 4  # (paths of several lengths share a wavefront)


@pytest.mark.parametrize("limit", [None, 0.1])
def test_row_shape_behind_every_kind_of_stop(oracle_mod, pk, mode, limit):
    O = oracle_mod
    with O.math_mode(mode):
        ch, start, goals, out, held = oracle_offsets(O, pk, limit, mode == "portable")
    sol, st, cost, stats, reached, steps, fraction = out
    W = W_OFFSETS
    zero = np.zeros((), dtype=PR.STATS_DTYPE)
    for p in range(len(start)):
        n, r = int(steps[p]), int(reached[p])
        if n > W:
            assert r == 0 and fraction[p] == 0.0 and (st[p] == CR.NOT_ATTEMPTED).all() and (cost[p] == 0.0).all()
            np.testing.assert_array_equal(sol[p], np.tile(start[p], (W, 1)))
            assert (stats[p] == zero).all()
            continue
        assert (st[p, :r] > 0).all() and 0 <= r <= held[p] <= n
        last = sol[p, r - 1] if r > 0 else start[p]
        behind = r if r == n else r + 1  # (a complete path has no refused row)
        if r < n:
            assert st[p, r] in (pk.NO_IK_SOLUTION, pk.PATH_JUMP, pk.PATH_RELATIVE_JUMP), st[p, r]
            np.testing.assert_array_equal(sol[p, r], last)
            assert stats["cost_evals"][p, r] > 0 or st[p, r] != pk.PATH_RELATIVE_JUMP  # (its counters stay)
        assert (st[p, behind:] == CR.NOT_ATTEMPTED).all() and (cost[p, behind:] == 0.0).all()
        assert (stats[p, behind:] == zero).all()
        np.testing.assert_array_equal(sol[p, behind:], np.tile(last, (W - behind, 1)))
        # the two-factor formula
        want = np.float64(held[p]) / np.float64(n)
        if r < n and st[p, r] == pk.PATH_RELATIVE_JUMP:
            want = want * (np.float64(r + 1) / np.float64(held[p] + 1))
        else:
            assert r == held[p]
        assert fraction[p] == want, (p, fraction[p], want)


def test_relative_test_is_moveits():
    """checkRelativeJointSpaceJump on a hand-made trajectory: steps 1, 1, 4, 1 (mean 1.75): factor 2 trips at index 2,
    factor 3 not at all"""
    traj = np.array([[0.0, 0.0], [1.0, 0.0], [1.0, 1.0], [3.0, -1.0], [3.0, 0.0]])
    assert CR.relative_jump(traj, 2.0) == 2
    assert CR.relative_jump(traj, 3.0) is None
    assert CR.relative_jump(traj[:2], 1.0) is None  # (one step is its own mean)


@pytest.mark.parametrize("frame", [0, 1])
def test_rotating_fixtures_have_both_branches(oracle_mod, pk, mode, frame):
    O = oracle_mod
    ch = pk.robots.panda()
    o = O.Oracle(ch)
    with O.math_mode(mode):
        start, target = CR.rotating(ch, o.fk, frame)
        c = pk.Cartesian(frame=frame, max_rotation=0.05, min_steps=3)
        goals, steps = pk.interpolate_poses(c, o.fk(start), target, 16, strict=mode == "portable")
        po = O.default_params(mode=1)
        out, held = CR.reference_cartesian(lambda g, sd: o.solve_batch(po, g, sd, num_threads=O.max_threads()), goals,
                                           steps, start)
    cl = CR.classes(out, held, 16)
    print(f"rotating frame {frame} [{mode}] steps {steps.min()}..{steps.max()}: {cl}")
    assert cl[0] >= 1 and cl[1] + cl[4] >= 1, cl


# ---- declarations, bindings, build ----------------------------------------------------------------
def test_header_and_bindings_declare_the_entry_points(pk):
    header = open(os.path.join(ROOT, "include", "pick_ik_amd.h")).read()
    begin, end = header.index("[host-api-begin]"), header.index("[host-api-end]")
    for name in SYMBOLS + ("PIKAMD_PATH_RELATIVE_JUMP", "PIKAMD_CARTESIAN_GLOBAL", "PIKAMD_CARTESIAN_TIP",
                           "PIKAMD_CARTESIAN_OFFSET", "typedef struct pikamd_cartesian"):
        m = re.search(r"\b" + name + r"\b", header)
        assert m and begin < m.start() < end, name
    said = " ".join(header[begin:end].replace(" *", " ").split())
    for text in ("pose0 = pikamd_fk_batch(s, P, start)", "every steps[p] equals W", "compared unwrapped",
                 "are the caller's max_joint_step", "a validity callback"):
        assert text in said, text
    mirror = open(os.path.join(ROOT, "pick_ik_amd", "host", "pick_ik_amd.hpp")).read()
    assert "compute_cartesian_paths(" in mirror and "pikamd_cartesian_paths(" in mirror
    from pick_ik_amd import solver
    for strict in (False, True):
        L = solver.lib(strict)
        for name in SYMBOLS:
            assert name in solver.EXPORTED_SYMBOLS
            assert getattr(L, name).argtypes is not None, name
    for name in ("cartesian_paths", "cartesian_paths_device", "cartesian_kernel_name"):
        assert callable(getattr(pk.Solver, name))
    assert callable(pk.interpolate_poses)
    assert (pk.PATH_RELATIVE_JUMP, pk.CARTESIAN_GLOBAL, pk.CARTESIAN_TIP, pk.CARTESIAN_OFFSET) == (-1003, 0, 1, 2)
    assert C.sizeof(pk.Cartesian) == 32


def test_shape_checks_come_before_the_library(pk):
    """(no GPU here: a call that reached the library would fail for another reason)"""
    s = pk.Solver.__new__(pk.Solver)  # a handle-less object: the checks must raise before anything is called
    s.dof, s.n_tips, s._env_options = 7, 1, lambda: None
    p = pk.default_params(mode=1)
    c = pk.Cartesian(frame=2, max_translation=0.1)
    start, target = np.zeros((4, 7)), np.zeros((4, 7))
    with pytest.raises(ValueError, match="start"):
        s.cartesian_paths(p, c, np.zeros((4, 6)), target, 3)
    with pytest.raises(ValueError, match="start"):
        s.cartesian_paths(p, c, np.zeros(7), target, 3)
    with pytest.raises(ValueError, match="target"):
        s.cartesian_paths(p, c, start, np.zeros((3, 7)), 3)
    with pytest.raises(ValueError, match="target"):
        s.cartesian_paths(p, c, start, np.zeros((4, 6)), 3)
    with pytest.raises(ValueError, match="at least one waypoint"):
        s.cartesian_paths(p, c, start, target, 0)
    with pytest.raises(ValueError, match="max_joint_step"):
        s.cartesian_paths(p, c, start, target, 3, max_joint_step=np.zeros(6))
    with pytest.raises(ValueError, match="W >= 1"):
        s.cartesian_paths_device(p, c, 4, 0, 1, 1, 1, 1, 1)
    with pytest.raises(ValueError, match="start_pose"):
        pk.interpolate_poses(c, np.zeros((4, 6)), target, 3)
    with pytest.raises(ValueError, match="target"):
        pk.interpolate_poses(c, start, np.zeros((5, 7)), 3)
    with pytest.raises(ValueError, match="at least one waypoint"):
        pk.interpolate_poses(c, start, target, 0)
    s._h = None


def kernel_names(fl, d):
    names = [f"cartesian_prepare_kernel<{d}>", f"ik_cartesian_kernel<{d}>"]
    return names + ([f"ik_cartesian_wide_kernel<{d},{l}>" for l in (16, 8)] if fl == "fast"
                    else [f"ik_cartesian_team_kernel<{d},{l}>" for l in (16, 4)])


FLAVOURS = (("fast", "pik"), ("exact", "pik_exact"), ("strict", "pik_strict"))


def test_build_tables_name_the_family():
    from pick_ik_amd import build as Bd
    assert Bd.FAMILIES["pik_cartesian_inst.hip"] == (("fast", "exact"), ("strict",))
    assert "pik_cartesian_inst.hip" in Bd.APPENDED_FAMILIES
    for strict, flavours in ((False, ("fast", "exact")), (True, ("strict",))):
        objs = [o for o in Bd.link_objects(strict) if "pik_cartesian" in o[0]]
        assert objs == [o for fl in flavours for o in Bd.family_objects("pik_cartesian_inst.hip", fl)]
        assert Bd.link_objects(strict)[:len(Bd.library_objects(strict))] == Bd.library_objects(strict)


def test_committed_ledger_has_the_kernels():
    path = os.path.join(ROOT, "profiles", "r06_kernel_resources.csv")
    rows = {(r["flavour"], r["kernel"]): r for r in csv.DictReader(open(path))}
    n = [k for k in rows if "cartesian" in k[1]]
    assert len(n) == 16 * 4 * 3
    assert {fl for fl, _ in n} == {"fast", "exact", "strict"}
    for fl, ns in FLAVOURS:
        for d in range(1, 17):
            for k in kernel_names(fl, d):
                assert (fl, f"{ns}::{k}") in rows, (fl, k)
    # no name is counted by the tests of the other families
    for _, k in n:
        for other in ("::ik_path", "::ik_search", "::ik_startpath", "::ik_globalpath", "::search_finalize"):
            assert other not in k, (k, other)
    # a fast walk kernel spills no vector register and has no scratch, like its ik_path_* twin
    for fl, k in n:
        if fl == "fast" and "prepare" not in k:
            assert int(rows[(fl, k)]["vgpr_spills"]) == 0 and int(rows[(fl, k)]["scratch_bytes_per_lane"]) == 0, k


def test_the_kernels_are_reached_from_no_existing_translation_unit():
    from pick_ik_amd import build as Bd
    for tu in ("pik_inst.hip", "pik_path_inst.hip", "pik_search_inst.hip", "pik_route_inst.hip", "pik_restart_inst.hip",
               "pik_startpath_inst.hip", "pik_globalpath_inst.hip"):
        for f in Bd._deps(tu, True):
            assert "pik_cartesian" not in os.path.basename(f) and os.path.basename(f) != "pik_interp.hpp", (tu, f)
    ops = Bd._strip_comments(open(os.path.join(Bd.CSRC, "pik_cartesian_ops.hpp")).read())
    assert not re.search(r"__global__|__device__|__shared__|__constant__", ops)
    assert not any(os.path.basename(f) == "pik_cartesian.hpp" for f in Bd._deps("pik_amd.hip", True))
    # the interpolation is one header, read by the C ABI translation unit (host) and by the kernels (device)
    assert any(os.path.basename(f) == "pik_interp.hpp" for f in Bd._deps("pik_amd.hip", True))
    assert any(os.path.basename(f) == "pik_interp.hpp" for f in Bd._deps("pik_cartesian_inst.hip", True))


def test_a_hip_caller_compiles_against_the_header_and_the_mirror(tmp_path):
    """tests/native/cartesian_api_check.hip calls the four entry points and Solver::compute_cartesian_paths from a .hip
    file: hipcc compiles it for gfx950, device pass included"""
    from pick_ik_amd import build as Bd
    src = os.path.join(ROOT, "tests", "native", "cartesian_api_check.hip")
    r = subprocess.run([Bd.hipcc(), "--offload-arch=gfx950", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-c", src, "-o",
                        str(tmp_path / "cartesian_api_check.o")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]


def test_interpolation_header_under_the_sanitizers(tmp_path):
    """tests/native/interp_sanitize.cpp: a stand-alone program (its own main) over the interpolation header, built with
    -fsanitize=address,undefined and run directly over generated cases -- no Python inside, no preload"""
    from pick_ik_amd import build as Bd
    src = os.path.join(ROOT, "tests", "native", "interp_sanitize.cpp")
    exe = str(tmp_path / "interp_sanitize")
    clang = os.path.join(os.path.dirname(os.path.realpath(Bd.hipcc())), "..", "llvm", "bin", "clang++")
    cxx = clang if os.path.exists(clang) else "g++"
    r = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                        "-Wall", "-Wextra", "-Werror", "-Wno-unknown-pragmas", src, "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "interp sanitize OK" in r.stdout, r.stdout[-2000:] + r.stderr[-3000:]
