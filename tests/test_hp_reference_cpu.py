"""CPU: the high-precision reference (tests/hp_reference.py) itself -- against the oracle (math mode libm) at rounding
level on the reference robots and on generated chains of 1..16 variables, and against the upstream known answers the
oracle tests hold (tests/test_oracle_golden.py: frame tests, pose costs, the bio_ik samples, RR forward kinematics,
the Panda's ready height, the minimal displacement factors)."""
import math

import numpy as np
import pytest

from pick_ik_amd import robots
from tests import hp_reference as H
from tests import test_oracle_golden as G
from tests.test_gpu_fuzz import random_chain

U = H.EPS


def oracle_bound(ch, q):
    """the oracle's own rounding (libm sin / cos, the plain chain product): 8 (D + 2) u per step, times R for a
    position (tests/test_gpu_fk_accuracy.py)"""
    d = max(len(p.variable) for p in H.paths(ch))
    return 8 * (d + 2) * U * H.reach(ch, q), 8 * (d + 2) * U


CHAINS = [("panda", robots.panda), ("ur5", robots.ur5), ("rr", robots.rr), ("panda_on_torso", robots.panda_on_torso),
          ("torso_dual_arm", robots.torso_dual_arm)] + \
         [(f"random_{d}", (lambda d=d: random_chain(np.random.default_rng(900 + d), d))) for d in range(1, 17)]


@pytest.mark.parametrize("name,make", CHAINS, ids=[c[0] for c in CHAINS])
def test_fk_agrees_with_the_oracle(oracle_mod, name, make):
    O = oracle_mod
    ch = make()
    o = O.Oracle(ch)
    rng = np.random.default_rng(3)
    lo = np.where(ch.bounded == 1, ch.qmin, -3.0)
    hi = np.where(ch.bounded == 1, ch.qmax, 3.0)
    q = rng.uniform(lo, hi, size=(12, ch.dof))
    with O.math_mode("libm"):
        f = o.fk(q)
    for i in range(len(q)):
        bp, ba = oracle_bound(ch, q[i])
        for dp, da, dn in H.pose_errors(ch, q[i], f[i]):
            assert dp <= bp and da <= ba, (name, i, dp, bp, da, ba)
            assert dn <= 8 * (ch.dof + 2) * U, (name, i, dn)  # the oracle's quaternion is unit to rounding


def test_fk_rejects_what_it_does_not_model():
    with pytest.raises(NotImplementedError):
        H.fk(robots.floating_panda(), np.zeros(14))


def pose(t, q):
    return list(t) + list(q)


IDENT = pose([0, 0, 0], [1, 0, 0, 0])


def hp_pose_cost(goal7, frame7, ps, rs):
    """pose cost between two poses given as x y z qw qx qy qz (the frame's rotation exact from its quaternion)"""
    lin = H.linear_distance([H.mpf(v) for v in frame7[:3]], goal7[:3])
    return H.pose_cost(lin, H.quat_angle(H.unit(frame7[3:]), H.unit(goal7[3:])), ps, rs)


def hp_frame_test(goal7, frame7, pe, oe):
    lin = H.linear_distance([H.mpf(v) for v in frame7[:3]], goal7[:3])
    ang = H.quat_angle(H.unit(frame7[3:]), H.unit(goal7[3:]))
    return (pe is None or lin <= pe) and (oe is None or ang <= oe)


def test_upstream_frame_tests():
    """tests/goal_tests.cpp:9-72 (tests/test_oracle_golden.py test_frame_tests)"""
    pe, oe = 0.00001, 0.001
    assert hp_frame_test(IDENT, IDENT, 0.0, 0.0)
    assert not hp_frame_test(IDENT, pose([pe, pe, pe], [1 - oe, 0, 0, oe]), pe, oe)
    assert not hp_frame_test(IDENT, pose([0, 0.000009, 0], [0.707, 0, 0.707, 0]), pe, oe)
    assert hp_frame_test(IDENT, pose([0, 0.000009, 0], [0.99999, 0, 0, 0.00001]), pe, oe)
    f = pose([0, 0, 0], G.angle_axis(math.pi / 4, [0, 0, 1]))
    assert not hp_frame_test(IDENT, f, pe, oe)
    assert hp_frame_test(IDENT, f, pe, None)


def test_upstream_pose_costs():
    """tests/goal_tests.cpp:74-169 and the bio_ik samples :171-225 (tests/test_oracle_golden.py)"""
    c = lambda f, ps, rs: float(hp_pose_cost(IDENT, f, ps, rs))  # noqa: E731
    one = [1, 0, 0, 0]
    assert c(IDENT, 1.0, 0.5) == 0.0
    assert c(pose([0, 2, 0], one), 1.0, 0.5) == pytest.approx(4.0, rel=1e-15)
    assert c(pose([1, 1, 0], one), 1.0, 0.5) == pytest.approx(2.0, rel=1e-15)
    assert c(pose([1, 1, 1], one), 1.0, 0.5) == pytest.approx(3.0, rel=1e-15)
    assert c(pose([1, 1, 1], one), 0.0, 0.5) == 0.0
    assert c(pose([0, 0, 0], G.angle_axis(1.0, [1, 0, 0])), 1.0, 0.0) == 0.0
    ry2 = pose([0, 0, 0], G.angle_axis(2.0, [0, 1, 0]))
    assert c(ry2, 1.0, 1.0) == pytest.approx(4.0, rel=1e-15)
    assert c(ry2, 1.0, 0.5) == pytest.approx(1.0, rel=1e-15)
    for case in G.BIO_IK_CASES:
        goal = pose(case["goal_t"], G.BIO_IK_GOAL_Q)
        frame = pose(case["frame_t"], case["frame_q"])
        dt = np.array(case["goal_t"]) - np.array(case["frame_t"])
        dot = float(np.dot(G.BIO_IK_GOAL_Q, case["frame_q"]))
        expected = float(dt @ dt) + (2.0 * math.acos(dot) * 0.5) ** 2
        assert float(hp_pose_cost(goal, frame, 1.0, 0.5)) == pytest.approx(expected, rel=1.19e-5)
        assert float(hp_pose_cost(goal, goal, 1.0, 0.5)) == 0.0


def test_upstream_rr_fk_and_panda_height():
    """tests/ik_tests.cpp:50-75; the bio_ik goals' height (tests/goal_tests.cpp:177) and the ready pose's tool axis"""
    (t, _), = H.fk(robots.rr(2.0, 1.0), [0.0, 0.0])
    assert float(t[0]) == 3.0 and float(t[1]) == 0.0
    (t, _), = H.fk(robots.rr(2.0, 1.0), [math.pi / 4, -math.pi / 4])
    assert float(t[0]) == pytest.approx(2.0 * math.cos(math.pi / 4) + 1.0, rel=1e-15)
    assert float(t[1]) == pytest.approx(2.0 * math.sin(math.pi / 4), rel=1e-15)
    p = H.pose7(robots.panda(), robots.PANDA_HOME)
    assert p[2] == pytest.approx(0.5902695655822754, abs=2e-5)
    assert abs(p[4]) == pytest.approx(1.0, abs=1e-15)


def test_minimal_displacement_factors_and_joint_goals(oracle_mod):
    """Robot::from (src/robot.cpp:44-85) and the three joint goals (src/goal.cpp:91-144) against the oracle"""
    O = oracle_mod
    ch = random_chain(np.random.default_rng(4), 9)
    v = O.Oracle(ch).variables()
    for j, (b, mid, hs, f) in enumerate(H.variables(ch)):
        assert float(f) == pytest.approx(v[j, 5], rel=2e-16)
    o = O.Oracle(ch)
    rng = np.random.default_rng(5)
    kw = dict(center_joints_weight=0.3, avoid_joint_limits_weight=0.2, minimal_displacement_weight=0.1)
    p = O.default_params(**kw)
    for _ in range(8):
        q = rng.uniform(ch.qmin - 0.5, ch.qmax + 0.5)
        seed = rng.uniform(ch.qmin, ch.qmax)
        terms = H.joint_goal_terms(ch, p, seed, q)
        want = [o.center_joints_cost(q), o.avoid_joint_limits_cost(q), o.minimal_displacement_cost(q, seed)]
        for (w, t), x in zip(terms, want):
            assert float(t) == pytest.approx(x, rel=1e-14, abs=1e-300)
        goal = o.fk(q + 0.01)[0]
        with O.math_mode("libm"):
            c, sol = o.cost(p, goal, seed, q)
        r = H.cost(ch, p, goal, seed, q)
        assert float(r.cost) == pytest.approx(c[0], rel=1e-12)
        assert r.solution == bool(sol[0])


@pytest.mark.parametrize("mode", ["libm", "portable", "fma"])
@pytest.mark.parametrize("name,h", [("panda", 1e-4), ("ur5", 1e-12), ("rr", 0.3), ("random_8", 3e-2)])
def test_step_agrees_with_the_oracle(oracle_mod, mode, name, h):
    """hp_reference.step against the oracle's literal step() (pko_gd_step_batch) in its three math modes: the
    normalised gradient, the update from the oracle's own gradient and the cost there within the bounds of
    tests/test_gpu_step_accuracy.py for an exact flavour (the oracle's chain product: 8 (D + 2) u per step)"""
    from tests import test_gpu_step_accuracy as S
    O = oracle_mod
    ch = random_chain(np.random.default_rng(908), 8) if name == "random_8" else robots.by_name(name)
    o = O.Oracle(ch)
    rng = np.random.default_rng(31)
    n = 6
    lo = np.where(ch.bounded == 1, ch.qmin, -3.0)
    hi = np.where(ch.bounded == 1, ch.qmax, 3.0)
    q = rng.uniform(lo, hi, size=(n, ch.dof))
    seed = rng.uniform(lo, hi, size=(n, ch.dof))
    with O.math_mode(mode):
        goal = o.fk(rng.uniform(lo, hi, size=(n, ch.dof)))
        p = O.default_params(gd_step_size=h, center_joints_weight=0.05, avoid_joint_limits_weight=0.1,
                             minimal_displacement_weight=0.02)
        lc = np.array([o.cost(p, goal[i], seed[i], q[i])[0][0] for i in range(n)])
        local, best, lc2, bc, G, imp = o.gd_step(p, goal, seed, q, q, lc, lc)
    asserted = 0
    for i in range(n):
        st = H.step(ch, p, goal[i], seed[i], q[i], G=G[i])
        eg = S.gradient_bounds(ch, p, "exact", q[i], seed[i], st)
        eG = S.normalised_bounds(st, eg, h)
        assert (np.abs(G[i] - [float(x) for x in st.G]) <= eG).all(), (name, mode, i)
        ep2, ecd = S.line_bounds(ch, p, "exact", q[i], st.ls, 1)
        cd, jd = abs(float(st.ls.cost_diff)), abs(float(st.ls.joint_diff))
        if cd > 2 * ecd:
            asserted += 1
            ejd = (ep2 + jd * ecd) / (cd - ecd) + 2 * U * jd
            eq = np.abs(G[i]) * ejd + 2 * U * (np.abs(q[i]) + np.abs(G[i]) * jd)
            assert (np.abs(local[i] - [float(x) for x in st.ls.local]) <= eq).all(), (name, mode, i)
        r = H.cost(ch, p, goal[i], seed[i], local[i])
        assert abs(lc2[i] - float(r.cost)) <= S.cost_bound(ch, p, "exact", local[i], r), (name, mode, i)
    assert asserted >= n // 2, (name, mode, asserted)


def test_off_unit_goal_quaternions_agree_with_the_oracle(oracle_mod):
    """hp_reference.goal_quat -- a goal quaternion off unit norm taken as upstream takes it (tf2::fromMsg's
    toRotationMatrix, which does not normalise, then Quaterniond(matrix) by Eigen's branches) -- against the oracle,
    whose make_goal restates the same path: the cost agrees to rounding, on both of Eigen's branches (trace > 0 and
    the largest diagonal entry), while the normalised quaternion would give another cost"""
    O = oracle_mod
    ch = robots.panda()
    o = O.Oracle(ch)
    rng = np.random.default_rng(43)
    n = 24
    q = rng.uniform(ch.qmin, ch.qmax, size=(n, ch.dof))
    goal = np.array([H.pose7(ch, x) for x in rng.uniform(ch.qmin, ch.qmax, size=(n, ch.dof))])
    goal[:, 3:] *= np.array([1.1, 0.9, 1 + 1e-3, 1 - 1e-3, 1 + 1e-6, 1 - 1e-6] * 4)[:, None]
    p = O.default_params()
    branches, differs = set(), 0
    for i in range(n):
        w, x, y, z = goal[i, 3:]
        branches.add(3 - 4 * (x * x + y * y + z * z) > 0)  # the trace of toRotationMatrix
        with O.math_mode("libm"):
            c = o.cost(p, goal[i], q[i], q[i])[0][0]
        r = H.cost(ch, p, goal[i], q[i], q[i])
        assert float(r.cost) == pytest.approx(c, rel=1e-12), (i, float(r.cost), c)
        (t, R), = H.fk(ch, q[i])
        unit = H.pose_cost(H.linear_distance(t, goal[i, :3]), H.quat_angle(H.matrix_to_quat(R), H.unit(goal[i, 3:])),
                           p.position_scale, p.rotation_scale)
        differs += abs(float(unit) - c) > 1e-9 * c
    assert branches == {True, False}, branches
    assert differs >= 8, differs
