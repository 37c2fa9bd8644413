"""CPU: the high-precision reference (tests/hp_reference.py) itself -- against the oracle (math mode libm) at rounding
level on the reference robots and on generated chains of 1..16 variables, and against the upstream known answers the
oracle tests hold (tests/test_oracle_golden.py: frame tests, pose costs, the bio_ik samples, RR forward kinematics,
the Panda's ready height, the minimal displacement factors).  Chains with a floating joint or with mimic joints: the
checks of tests/test_gpu_floating_mimic_accuracy.py -- FK, cost and verdict, step() stage by stage, the same samples,
edges and bounds -- run here on the oracle in its three math modes, which the exact kernels repeat bit for bit."""
import dataclasses
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
    """a floating joint is seven consecutive variables in MoveIt's order (tests/test_floating_cpu.py
    test_chain_description_validates_floating_joints); a mimic joint follows a joint of its path"""
    ch = robots.floating_panda()
    assert len(H.paths(ch)) == 1
    bad = ch.joint_type.copy()
    bad[3] = robots.REVOLUTE  # a hole in the seven variables
    with pytest.raises(ValueError, match="floating joint"):
        H.fk(dataclasses.replace(ch, joint_type=bad), np.zeros(14))
    bad = ch.joint_type.copy()
    bad[:7] = bad[:7][::-1]  # wrong order
    with pytest.raises(ValueError, match="floating joint"):
        H.paths(dataclasses.replace(ch, joint_type=bad))
    bad = ch.joint_type.copy()
    bad[7:] = bad[:7]
    bad[13] = robots.REVOLUTE  # a second joint cut off after six of its variables
    with pytest.raises(ValueError, match="floating joint"):
        H.paths(dataclasses.replace(ch, joint_type=bad))
    m = robots.MimicJoint(after_variable=2, master_variable=8, origin_xyz_rpy=(0,) * 6, axis=(0, 0, 1))
    with pytest.raises(NotImplementedError):  # between the variables of the floating joint
        H.paths(dataclasses.replace(ch, mimic=(m,)))
    with pytest.raises(ValueError, match="mimic joint"):
        H.paths(dataclasses.replace(ch, mimic=(dataclasses.replace(m, after_variable=14),)))
    with pytest.raises(ValueError, match="mimic joint"):
        H.paths(dataclasses.replace(ch, mimic=(dataclasses.replace(m, after_variable=6, joint_type=robots.PLANAR_X),)))
    assert len(H.paths(dataclasses.replace(ch, mimic=(dataclasses.replace(m, after_variable=6),)))[0].mimic) == 1


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


# ---------------------------------------------------------------------------------------------------------------
# floating and mimic joints
# ---------------------------------------------------------------------------------------------------------------
MODES = ("libm", "portable", "fma")


class OracleHandle:
    """the oracle in one math mode behind the methods of pick_ik_amd.Solver that the accuracy checks call"""

    def __init__(self, O, ch, mode):
        self.O, self.o, self.mode = O, O.Oracle(ch), mode

    def _p(self, p):
        return self.O.Params.from_buffer_copy(bytes(p))

    def fk(self, q):
        with self.O.math_mode(self.mode):
            return self.o.fk(q)

    def cost(self, p, goal, seed, q):
        with self.O.math_mode(self.mode):
            r = [self.o.cost(self._p(p), goal[i], seed[i], q[i]) for i in range(len(q))]
        return np.array([x[0][0] for x in r]), np.array([x[1][0] for x in r])

    def gd_step(self, p, *a):
        with self.O.math_mode(self.mode):
            return self.o.gd_step(self._p(p), *a)

    def solve_batch(self, p, goal, seed, rng_seed=0):
        with self.O.math_mode(self.mode):
            return self.o.solve_batch(self._p(p), goal, seed, rng_seed=rng_seed, num_threads=self.O.max_threads())

    def kernel_name(self, p):
        return "pik_exact::(the oracle)"

    def close(self):
        pass


@pytest.fixture
def F(oracle_mod, monkeypatch):
    """tests/test_gpu_floating_mimic_accuracy.py with the oracle (flavour = math mode) in place of the GPU handles"""
    from tests import test_gpu_fk_accuracy as A
    from tests import test_gpu_floating_mimic_accuracy as F
    from tests import test_gpu_step_accuracy as S
    handle = lambda ch, mode: OracleHandle(oracle_mod, ch, mode)  # noqa: E731
    monkeypatch.setattr(A, "solver", handle)
    monkeypatch.setattr(S, "solver", handle)
    F.handle = handle
    return F


def test_the_floating_chains_are_what_they_are_meant_to_be(F):
    for name, where in (("floating_middle", "middle"), ("floating_end", "end")):
        ch = F.chain(name)
        at = int(np.flatnonzero(ch.joint_type == robots.FLOATING_TX)[0])
        assert 1 <= ch.dof - 7 <= 9 and (0 < at < ch.dof - 7 if where == "middle" else at == ch.dof - 7), (name, at)
    two = F.chain("two_tip_floating")
    assert [list(t.variable[:7]) for t in two.tips] == [list(range(7))] * 2
    for name in F.FLOATING:  # the edges are in every batch, and at least half of it is uniform
        ch = F.chain(name)
        q = F.samples(name, 21)
        quat = F.floating_blocks(ch)[0][3:]
        s2 = (q[11:, quat] ** 2).sum(axis=1)
        assert (s2 == 4).any() and (s2 == 0).any() and ((s2 > 0) & (s2 < 1e-15)).any() and (abs(s2 - 1) < 1e-15).any()
        margins = [min(float(m) for m, _ in H.branch_decisions(R)) for x in q[11:] for _, R in H.fk(ch, x)[:1]]
        assert sum(m <= 1e-9 for m in margins) >= 2, (name, margins)  # (one by the trace, one by the diagonal)


def test_the_two_tip_floating_chain_is_accepted(F):
    """pikamd_create_multi validates the description before it looks for a device"""
    import torch
    import pick_ik_amd as pk
    try:
        pk.Solver(F.chain("two_tip_floating"), device=0).close()
    except pk.PickIkAmdError as e:
        assert not torch.cuda.is_available() and "no HIP device" in str(e), e


@pytest.mark.parametrize("n", [21, 65])
@pytest.mark.parametrize("name", ["floating_panda", "floating_middle", "floating_end", "two_tip_floating"])
def test_floating_fk_agrees_with_the_oracle(F, name, n):
    """position and every quaternion component, Eigen's sign and branch included"""
    r = F.check_fk_components(name, n, flavours=MODES, handle=F.handle)
    assert all(v["on_a_decision"] >= 1 for v in r.values()), r


MIMIC_CASES = {f"{c[0]}_{c[1]}": c for c in __import__("tests.test_mimic_cpu", fromlist=["CASES"]).CASES}


def mimic_chain(key):
    """(the chain with the mimic joint, the chain with it as a variable, q -> that chain's q)"""
    from tests import test_mimic_cpu as T
    if key == "prismatic_two_in_a_row":
        return T.prismatic_and_two_in_a_row()
    name, k, master, mult, off = MIMIC_CASES[key]
    full = robots.by_name(name)
    ch, keep = T.with_mimic(None, full, k, master, mult, off)
    return ch, full, lambda q: T.expand(q, keep, k, master, mult, off, full.dof)


@pytest.mark.parametrize("key", list(MIMIC_CASES) + ["prismatic_two_in_a_row"])
def test_mimic_fk_and_cost_agree_with_the_oracle(F, oracle_mod, key):
    """the oracle's mimic step within the rounding bounds of the reference's, the cost and the verdict with it; and
    the identity: the reference equals itself on the chain with the joint as an ordinary variable (the double
    rounding of multiplier * master + offset, which that chain's joint vector holds, apart)"""
    from tests import test_gpu_fk_accuracy as A
    from tests import test_gpu_step_accuracy as S
    ch, full, as_variables = mimic_chain(key)
    rng = np.random.default_rng(17)
    n = 16
    q = rng.uniform(ch.qmin, ch.qmax, size=(n, ch.dof))
    q[0], q[1] = ch.qmin, ch.qmax
    print(key, A.check_fk(ch, q, flavours=MODES, what=key))
    qf = as_variables(q)
    slack = sum(2 * U * (abs(m.multiplier) * 3.8 + abs(m.offset)) for m in ch.mimic)
    for i in range(n):
        (t, R), (tf, Rf) = H.fk(ch, q[i])[0], H.fk(full, qf[i])[0]
        assert max(abs(float(a - b)) for a, b in zip(t, tf)) <= slack * H.reach(full, qf[i]), (key, i)
        assert max(abs(float(a - b)) for ra, rb in zip(R, Rf) for a, b in zip(ra, rb)) <= slack, (key, i)
    import pick_ik_amd as pk
    p = pk.default_params(**F.COST_KW)
    goal = A.goals_around(ch, q, rng)
    seed = rng.uniform(ch.qmin, ch.qmax, size=(n, ch.dof))
    refs = [H.cost(ch, p, goal[i], seed[i], q[i]) for i in range(n)]
    for mode in MODES:
        c, sol = OracleHandle(oracle_mod, ch, mode).cost(p, goal, seed, q)
        for i, r in enumerate(refs):
            assert abs(c[i] - float(r.cost)) <= S.cost_bound(ch, p, "exact", q[i], r), (key, mode, i)
            assert bool(sol[i]) == r.solution, (key, mode, i)


@pytest.mark.parametrize("name,n", [("floating_panda", 33), ("floating_middle", 21), ("floating_end", 65),
                                    ("two_tip_floating", 21), ("mimic_revolute", 33), ("mimic_prismatic", 65)])
def test_floating_and_mimic_cost_agrees_with_the_oracle(F, name, n):
    F.check_cost(name, n, flavours=MODES, handle=F.handle)


@pytest.mark.parametrize("name,h,n", [("floating_panda", 1e-4, 33), ("floating_middle", 1e-8, 33),
                                      ("floating_end", 0.3, 65), ("two_tip_floating", 1e-8, 21),
                                      ("mimic_revolute", 0.3, 33), ("mimic_prismatic", 1e-4, 33)])
def test_floating_and_mimic_step_agrees_with_the_oracle(F, name, h, n):
    """tests/test_gpu_step_accuracy.py check() on the oracle's step(): every stage within its bound, the line search
    asserted for at least half of the samples"""
    from tests import test_gpu_step_accuracy as S
    S.check(f"{name}-{h:g}-{n}", F.step_case(name, h, n), flavours=MODES)


@pytest.mark.parametrize("how", ["local", "memetic"])
@pytest.mark.parametrize("name", ["floating_panda", "mimic_revolute"])
def test_floating_and_mimic_solves_agree_with_the_oracle(F, name, how):
    """every SUCCESS a solution for the reference, every returned cost the reference's, and some problem solved"""
    F.check_solves(name, how, flavours=MODES, handle=F.handle)


def toy_floating_joint():
    """a floating joint alone: no other joint, identity origins"""
    return robots._chain("floating", np.zeros((7, 6)), np.tile([0.0, 0.0, 1.0], (7, 1)), np.zeros(6), [-1.0] * 7,
                         [1.0] * 7, [1.0] * 7, joint_type=np.array(robots.FLOATING, dtype=np.int32))


def test_a_floating_joint_alone_is_upstreams_formula():
    """Translation(v0 v1 v2) * Quaterniond(v6, v3, v4, v5) (src/forward_kinematics.cpp:64-70), the quaternion not
    normalised: for a quaternion of norm s and rotation R' (Rodrigues, from its angle and axis) the frame is
    s^2 R' + (1 - s^2) I -- R' itself for s = 1 -- and the translation is the three variables"""
    ch = toy_floating_joint()
    rng = np.random.default_rng(8)
    one = H.M.mpf(1)
    for norm in [1.0] * 6 + [2.0] * 6 + [1e-3, 1e-8, 1e-30, 1e-200, 0.0]:
        v = rng.normal(size=4)
        v *= norm / np.linalg.norm(v)
        x = np.concatenate([rng.uniform(-1, 1, size=3), v])
        (t, R), = H.fk(ch, x)
        assert [float(a) for a in t] == list(x[:3])
        qx, qy, qz, qw = (H.mpf(a) for a in v)  # (the variables hold x y z w)
        s2 = qw * qw + qx * qx + qy * qy + qz * qz
        nv = H.M.sqrt(qx * qx + qy * qy + qz * qz)
        Rp = H.rodrigues([qx / nv, qy / nv, qz / nv], 2 * H.M.atan2(nv, qw)) if nv > 0 else H._ident()
        for i in range(3):
            for j in range(3):
                want = s2 * Rp[i][j] + (1 - s2) * (one if i == j else 0)
                assert abs(R[i][j] - want) <= H.M.mpf(2) ** -120 * max(1, s2), (norm, i, j)
        if norm == 1.0:
            assert max(abs(float(R[i][j] - Rp[i][j])) for i in range(3) for j in range(3)) <= 8 * U
        if norm < 1e-7:  # the identity to rounding: the trace branch, w = 1
            qt, branch = H.frame_quat(R)
            assert branch == "w" and abs(float(qt[0]) - 1) <= 2 * norm ** 2


def test_frame_quat_on_rotations_is_matrix_to_quat():
    """for an exact rotation Eigen's branches give the unit quaternion of matrix_to_quat (the largest of the four
    candidates) up to sign, on every branch: the accuracy tests of the other chains do not move"""
    rng = np.random.default_rng(9)
    seen = set()
    for name in ("panda", "ur5", "torso_dual_arm"):
        ch = robots.by_name(name)
        for x in rng.uniform(ch.qmin, ch.qmax, size=(40, ch.dof)):
            for _, R in H.fk(ch, x):
                a, branch = H.frame_quat(R)
                b = H.matrix_to_quat(R)
                sign = 1 if a[0] * b[0] + a[1] * b[1] + a[2] * b[2] + a[3] * b[3] > 0 else -1
                assert max(abs(float(x - sign * y)) for x, y in zip(a, b)) <= 1e-35, (name, branch)
                assert a["wxyz".index(branch)] > 0
                seen.add(branch)
                for forced in "wxyz":  # (any branch whose square root does not vanish)
                    c = H.frame_quat(R, forced)[0]
                    if abs(c["wxyz".index(forced)]) > 1e-3:
                        assert max(abs(abs(float(x)) - abs(float(y))) for x, y in zip(a, c)) <= 1e-30
    assert seen == set("wxyz"), seen


def test_branch_decisions():
    """the margins of the comparisons taken, and where the other outcome of each leads"""
    d = lambda a, b, c: [[H.mpf(a), 0, 0], [0, H.mpf(b), 0], [0, 0, H.mpf(c)]]  # noqa: E731
    assert H.frame_quat(d(1, 1, 1))[1] == "w"
    assert [(float(m), o) for m, o in H.branch_decisions(d(0.5, -0.25, -0.125))] == [(0.125, "x")]
    assert H.frame_quat(d(0.25, -0.5, -0.75))[1] == "x"
    assert [(float(m), o) for m, o in H.branch_decisions(d(0.25, -0.5, -0.75))] == [(1.0, "w"), (0.75, "y"), (1.0, "z")]
    assert H.frame_quat(d(-0.5, -0.5, -0.5))[1] == "x"  # ties stay with the earlier entry, a trace of 0 goes by diagonal
    assert H.frame_quat(d(0.5, 0.0, -0.5))[1] == "x"
    assert [o for _, o in H.branch_decisions(d(-0.5, -0.25, 0.5))] == ["w", "z", "y"]
    assert H.frame_quat(d(-0.5, -0.25, 0.5))[1] == "z"
