"""Solver.gd_step -- one step() of src/ik_gradient.cpp:24-94 -- of the three libraries, exact (the default), fast
(exact=False) and strict (strict=True), against the high-precision step of tests/hp_reference.py, stage by stage,
within bounds from error analysis.  e_c(x) is the cost bound of tests/test_gpu_fk_accuracy.py at the point x
(per tip: 2 s_p^2 |dp| e_p + s_p^2 e_p^2 + 2 s_r^2 ang e_a + s_r^2 e_a^2 with e_p, e_a from fk_bounds, e_a +=
EXTRACT; plus 16 u of the cost); R' = max(R, 1) with R = hp_reference.reach(); u = 2^-53.

  gradient, literal kernels  g_j = c(fl(q_j + h)) - c(fl(q_j - h)) as the literal difference of two costs (the exact
                             flavours, and the fast one above h = 1e-2): e_g = e_c(+) + e_c(-) + u |g_j|
  gradient, fast flavour     h <= 1e-2: the difference term by term (pik_math.hpp probe_joint), per tip k:
      position     4 h s_p^2 (e_p R' + |dp_k| (e_a R' + 2 e_p) + 16 u |dp_k| R')    (the triple product
                   dt0 . (a x r) from a tip, an axis and an origin each off by e_p / e_a, |r| <= R')
      orientation  4 s_r^2 (H (e_A + 2 e_d) + (ang_k + H) 2 e_d + 4 u H (ang_k + H)),  H = min(h, pi),
                   e_A = e_a + EXTRACT the angle's error, e_d = (1 + h) e_A + 16 u the error of each half-angle
                   difference delta(+-) (the relative rotation off by e_A, the axis by e_a over the angle h; the
                   sine-of-a-difference form cancels to a few u absolute)
      joint goals  w^2 (2 (|t+| + |t-|) e_t + 2 e_t^2 + 4 u (t+^2 + t-^2)),  e_t = 4 u m (|q_j| + |mid| + hspan + h
                   + |seed_j|), per enabled goal (t+- the goal's term at fl(q_j +- h))
      exact h      the probes rotate by exactly h where the reference moves to the double fl(q_j +- h):
                   L (|fl(q_j + h) - (q_j + h)| + |fl(q_j - h) - (q_j - h)|), exact on the mpmath side, with L =
                   sum_k 2 (s_p^2 (|dp_k| + h R') R' + s_r^2 (ang_k + h)) >= |dc / dq_j| near q
  normalised gradient        G_j = g_j f, f = h / (h + sum |g|):
                             e_G = f e_g + |G_j| (sum_j e_g / (h + sum |g|) + (D + 4) u)
  line search                from the kernel's own G: p1, p3 at fl(q -+ G), each off by e_c (+ for the fast
                             flavour's angle addition, h <= 1e-3 and one tip: L |fl(q -+ G) - (q -+ G)| summed over
                             the joints); p2 = (p1 + p3) / 2 and cost_diff = (p3 - p1) / 2 off by
                             e = (e_1 + e_3) / 2 + u |.|;
                             e_jd = (e(p2) + |jd| e(cost_diff)) / (|cost_diff| - e(cost_diff)) + 2 u |jd|
                             (= |jd| (e(p2) / |p2| + e(cost_diff) / |cost_diff|) to first order), asserted where
                             |cost_diff| > 2 e(cost_diff); the other samples are counted, and every case asserts a
                             minimum share of asserted ones
  update                     clamp(q_j - G_j jd): |G_j| e_jd + 2 u (|q_j| + |G_j jd|) (the clamp is 1-Lipschitz)
  local_cost                 e_c at the returned joint vector
  best, best_cost, improved  exactly what local_cost < best_cost (the kernel's own numbers) implies

The fast flavour's probes take the arcsine of a half-angle difference as a 4-term series, exact to rounding up to
h = 1e-2 and off by h^8 above it (8e-9 of the gradient at h = 0.3): they missed their bound from h = 0.1 on, so a
larger step now takes the literal kernels (asserted here through Solver.kernel_name).  The measured worst fractions
of the bounds are printed per flavour and stage (DESIGN.md section 3 records them).
"""
import dataclasses
import math
import zlib

import numpy as np
import pytest

import pick_ik_amd as pk
from pick_ik_amd import robots
from tests import hp_reference as H
from tests.test_gpu_fk_accuracy import EXTRACT, FLAVOURS, angle_bounds, fk_bounds, solver
from tests.test_gpu_fuzz import random_chain

pytestmark = pytest.mark.gpu

U = H.EPS
LITERAL_ABOVE = 1e-2  # a larger gd_step_size is served by the literal kernels in every flavour (pik_amd.hip needs_literal)
GOALS = dict(center_joints_weight=0.05, avoid_joint_limits_weight=0.1, minimal_displacement_weight=0.02)


# ---------------------------------------------------------------------------------------------------------------
# bounds (see the module docstring)
# ---------------------------------------------------------------------------------------------------------------
def cost_bound(ch, p, fl, x, r):
    """e_c: the error of a flavour's cost at the joint vector x, r = hp_reference.cost there"""
    ep = fk_bounds(ch, x, fl)[0]
    sp2, sr2 = max(p.position_scale, 0.0) ** 2, max(p.rotation_scale, 0.0) ** 2
    t = 16 * U * float(r.cost)
    for lin, ang, ea in zip(r.lin, r.ang, angle_bounds(ch, x, fl, r)):
        t += 2 * sp2 * float(lin) * ep + sp2 * ep * ep + 2 * sr2 * float(ang) * ea + sr2 * ea * ea
    return t


def lipschitz(ch, p, r, h):
    """L >= |dc / dq_j| of the pose cost within h of the point of r (any joint)"""
    R = max(H.reach(ch), 1.0)
    sp2, sr2 = max(p.position_scale, 0.0) ** 2, max(p.rotation_scale, 0.0) ** 2
    return sum(2 * (sp2 * (float(lin) + h * R) * R + sr2 * (float(ang) + h)) for lin, ang in zip(r.lin, r.ang))


def off(a, b):
    """|fl(a + b) - (a + b)|, exact"""
    return float(abs(H.mpf(a + b) - (H.mpf(a) + H.mpf(b))))


def goal_probe_bound(ch, p, q, seed, j, h):
    """the joint goals' share of the fast flavour's probe error for joint j"""
    var = H.variables(ch)
    b, mid, hs, m = var[j]
    mid, hs, m = float(mid), float(hs), float(m)
    qp, qm = q[j] + h, q[j] - h
    et = 4 * U * m * (abs(q[j]) + abs(mid) + hs + h + abs(seed[j]))
    terms = []
    if p.center_joints_weight > 0 and b:
        terms.append((p.center_joints_weight, (qp - mid) * m, (qm - mid) * m))
    if p.avoid_joint_limits_weight > 0 and b:
        terms.append((p.avoid_joint_limits_weight, max(0.0, abs(qp - mid) * 2 - hs) * m,
                      max(0.0, abs(qm - mid) * 2 - hs) * m))
    if p.minimal_displacement_weight > 0:
        terms.append((p.minimal_displacement_weight, (qp - seed[j]) * m, (qm - seed[j]) * m))
    return sum(w * w * (2 * (abs(tp) + abs(tm)) * et + 2 * et * et + 4 * U * (tp * tp + tm * tm))
               for w, tp, tm in terms)


def gradient_bounds(ch, p, fl, q, seed, st, literal=None):
    """e_g per joint (the raw gradient p3 - p1) of one flavour, st = hp_reference.step; literal: the probes are the
    literal difference of two costs (default: what serves the flavour at this step size)"""
    h = p.gd_step_size
    out = []
    if literal is None:
        literal = fl != "fast" or h > LITERAL_ABOVE
    if literal:
        for j, (lo, hi) in enumerate(st.probes):
            xl, xh = q.copy(), q.copy()
            xl[j] -= h
            xh[j] += h
            out.append(cost_bound(ch, p, fl, xl, lo) + cost_bound(ch, p, fl, xh, hi) + U * abs(float(st.raw[j])))
        return np.array(out)
    ep, ea = fk_bounds(ch, q, fl)
    eA = ea + EXTRACT
    R = max(H.reach(ch, q), 1.0)
    hh = min(h, math.pi)
    ed = (1 + h) * eA + 16 * U
    sp2, sr2 = max(p.position_scale, 0.0) ** 2, max(p.rotation_scale, 0.0) ** 2
    pose = 0.0
    for lin, ang in zip(st.base.lin, st.base.ang):
        lin, ang = float(lin), float(ang)
        if p.position_scale > 0:
            pose += 4 * h * sp2 * (ep * R + lin * (ea * R + 2 * ep) + 16 * U * lin * R)
        if p.rotation_scale > 0:
            pose += 4 * sr2 * (hh * (eA + 2 * ed) + (ang + hh) * 2 * ed + 4 * U * hh * (ang + hh))
    L = lipschitz(ch, p, st.base, h)
    for j in range(len(q)):
        exact_h = L * (off(q[j], h) + off(q[j], -h))
        out.append(pose + goal_probe_bound(ch, p, q, seed, j, h) + exact_h + 4 * U * abs(float(st.raw[j])))
    return np.array(out)


def normalised_bounds(st, eg, h):
    s = h + sum(abs(float(g)) for g in st.raw)
    f = float(st.f)
    return f * eg + np.abs([float(g) for g in st.G]) * (eg.sum() / s + (len(eg) + 4) * U)


def line_bounds(ch, p, fl, q, ls, n_tips):
    """(e(p2), e(cost_diff)) of the kernel's line search, ls = hp_reference.line_search from its G"""
    h, G = p.gd_step_size, ls.G_line
    e = []
    for sgn, r in zip((-1.0, 1.0), ls.line):
        x = q + sgn * G
        t = cost_bound(ch, p, fl, x, r)
        if fl == "fast" and h <= 1e-3 and n_tips == 1:  # angle addition from q by exactly +-G
            t += lipschitz(ch, p, r, h) * sum(off(q[j], sgn * G[j]) for j in range(len(q)))
        e.append(t)
    m = (e[0] + e[1]) / 2
    return m + U * abs(float(ls.p2)), m + U * abs(float(ls.cost_diff))


def frac(d, e):
    """the worst error as a fraction of its bound (a zero bound holds only a zero error, asserted by the caller)"""
    d, e = np.atleast_1d(d), np.atleast_1d(e)
    return float(max([0.0] + [a / b for a, b in zip(d, e) if b > 0]))


# ---------------------------------------------------------------------------------------------------------------
# the check
# ---------------------------------------------------------------------------------------------------------------
@dataclasses.dataclass
class Case:
    ch: object
    q: np.ndarray
    goal: np.ndarray
    seed: np.ndarray
    kw: dict
    literal: bool = False  # a chain that the literal (pik_exact::) kernels serve in every flavour, at every step size


REFS = {}  # (case id) -> [hp_reference.step without a given G]: computed once per module


def sample(ch, rng, n):
    lo = np.where(ch.bounded == 1, ch.qmin, -3.0)
    hi = np.where(ch.bounded == 1, ch.qmax, 3.0)
    return rng.uniform(lo, hi, size=(n, ch.dof))


def far_goals(ch, rng, n):
    return np.array([H.pose7(ch, x).ravel() for x in sample(ch, rng, n)])


def check(name, case, min_share=0.5, flavours=tuple(FLAVOURS)):
    ch, q, goal, seed = case.ch, case.q, case.goal, case.seed
    n, D = q.shape
    n_tips = len(getattr(ch, "tips", [None]))
    p = pk.default_params(**case.kw)
    h = p.gd_step_size
    if name not in REFS:
        REFS[name] = [H.step(ch, p, goal[i], seed[i], q[i]) for i in range(n)]
    refs = REFS[name]
    rng = np.random.default_rng(5)
    best_in = q + rng.uniform(-1e-3, 1e-3, size=q.shape)
    lc_in = np.array([float(r.base.cost) for r in refs])
    bc_in = lc_in * rng.choice([0.5, 1.0, 2.0], size=n)
    report = {}
    for flavour in flavours:
        # (the bounds of the kernels that serve the handle)
        fl = "exact" if case.literal and flavour == "fast" else flavour
        s = solver(ch, flavour)
        try:
            if flavour == "fast":
                assert s.kernel_name(p).startswith("pik_exact::") == (h > LITERAL_ABOVE or case.literal), \
                    (name, s.kernel_name(p))
            local, best, lc, bc, G, imp = s.gd_step(p, goal, seed, q, best_in, lc_in, bc_in)
        finally:
            s.close()
        worst = dict(G=0.0, q=0.0, cost=0.0)
        asserted = 0
        for i, r in enumerate(refs):
            eg = gradient_bounds(ch, p, fl, q[i], seed[i], r)
            eG = normalised_bounds(r, eg, h)
            dG = np.abs(G[i] - np.array([float(x) for x in r.G]))
            assert (dG <= eG).all(), (name, fl, i, "G", dG.tolist(), eG.tolist(), q[i].tolist())
            worst["G"] = max(worst["G"], frac(dG, eG))
            # line search and update from the kernel's own G
            ls = H.line_search(ch, p, goal[i], seed[i], q[i], G[i])
            ep2, ecd = line_bounds(ch, p, fl, q[i], ls, n_tips)
            cd, jd = abs(float(ls.cost_diff)), abs(float(ls.joint_diff))
            if cd > 2 * ecd:
                asserted += 1
                ejd = (ep2 + jd * ecd) / (cd - ecd) + 2 * U * jd
                eq = np.abs(G[i]) * ejd + 2 * U * (np.abs(q[i]) + np.abs(G[i]) * jd)
                dq = np.abs(local[i] - np.array([float(x) for x in ls.local]))
                assert (dq <= eq).all(), (name, fl, i, "update", dq.tolist(), eq.tolist())
                worst["q"] = max(worst["q"], frac(dq, eq))
            elif float(ls.cost_diff) == 0:
                # joint_diff not finite -> 0: the update is the clamp of q itself
                np.testing.assert_array_equal(local[i], [float(x) for x in ls.local], err_msg=f"{name} {fl} {i}")
            # local_cost: the reference cost at the returned joint vector
            rc = H.cost(ch, p, goal[i], seed[i], local[i])
            ec = cost_bound(ch, p, fl, local[i], rc)
            dc = abs(lc[i] - float(rc.cost))
            assert dc <= ec, (name, fl, i, "local_cost", lc[i], float(rc.cost), ec)
            worst["cost"] = max(worst["cost"], frac(dc, ec))
            # best / best_cost / improved from the kernel's own local_cost
            better = lc[i] < bc_in[i]
            assert imp[i] == int(better), (name, fl, i)
            np.testing.assert_array_equal(best[i], local[i] if better else best_in[i])
            assert bc[i] == (lc[i] if better else bc_in[i]), (name, fl, i)
        assert asserted >= min_share * n, (name, fl, asserted, n)
        report[flavour] = {k: round(v, 3) for k, v in worst.items()} | {"asserted": f"{asserted}/{n}"}
    print(name, f"h={h:g}", report)
    return report


# ---------------------------------------------------------------------------------------------------------------
# cases: a cross of robots, step sizes and edge states, 16-32 samples each
# ---------------------------------------------------------------------------------------------------------------
def planar_chain():
    from pick_ik_amd.urdf import chain_from_urdf
    from tests.test_planar_cpu import MOBILE
    return chain_from_urdf(MOBILE, "odom", "tool")


def rotate(qt, angle, axis):
    from tests.test_gpu_fk_accuracy import rotate as rot
    return rot(qt, angle, axis)


def near_pi_goals(ch, q, rng):
    """orientation error pi - 10^-k: |w0| -> 0 where the half-angle is reflected (fabs)"""
    g = np.array([H.pose7(ch, x) for x in q])
    for i in range(len(q)):
        ax = rng.normal(size=3)
        g[i, 3:] = rotate(g[i, 3:], math.pi - 10.0 ** -rng.uniform(1, 8), ax / np.linalg.norm(ax))
        g[i, :3] += rng.normal(size=3) * 0.05
    return g


def make_case(kind, h, n):
    rng = np.random.default_rng(zlib.crc32(f"{kind} {h!r}".encode()))
    kw = dict(gd_step_size=h)
    if kind == "panda_far":
        ch = robots.panda()
        q = sample(ch, rng, n)
        return Case(ch, q, far_goals(ch, rng, n), sample(ch, rng, n), kw)
    if kind == "panda_goals":  # joint goals on; q +- h across the avoid-limits kink and the centre
        ch = robots.panda()
        q = sample(ch, rng, n)
        var = H.variables(ch)
        mid = np.array([float(v[1]) for v in var])
        hs = np.array([float(v[2]) for v in var])
        q[: n // 3] = mid + hs / 2 * rng.choice([-1.0, 1.0], size=(n // 3, 7)) + rng.uniform(-h, h, size=(n // 3, 7))
        q[n // 3: 2 * n // 3] = mid + rng.uniform(-h, h, size=(2 * n // 3 - n // 3, 7))
        return Case(ch, q, far_goals(ch, rng, n), sample(ch, rng, n), kw | GOALS)
    if kind == "panda_near_pi":
        ch = robots.panda()
        q = sample(ch, rng, n)
        return Case(ch, q, near_pi_goals(ch, q, rng), q, kw)
    if kind == "ur5_limits":  # at a joint limit, goals far away: joint_diff large enough to clamp
        ch = robots.ur5()
        q = sample(ch, rng, n)
        k = rng.integers(0, 6, size=n)
        q[np.arange(n), k] = np.where(rng.uniform(size=n) < 0.5, ch.qmin[k], ch.qmax[k])
        return Case(ch, q, far_goals(ch, rng, n), q, kw | dict(avoid_joint_limits_weight=0.2))
    if kind == "rr_axis":  # the tip on (or 1e-9 .. 1e-3 off) the first joint's axis: equal links folded back
        ch = robots.rr(1.0, 1.0)
        q = np.stack([rng.uniform(-3, 3, size=n), math.pi - 10.0 ** -rng.uniform(3, 9, size=n)], axis=1)
        q[: n // 4, 1] = math.pi
        q = np.clip(q, ch.qmin, ch.qmax)
        return Case(ch, q, far_goals(ch, rng, n), q, kw)
    if kind == "random":  # arbitrary axes, prismatic and continuous joints; continuous ones beyond the fold
        ch = random_chain(np.random.default_rng(0x57E9), 8)
        q = sample(ch, rng, n)
        cont = np.nonzero((ch.bounded == 0) & (ch.joint_type == robots.REVOLUTE))[0]
        assert len(cont) and (ch.joint_type == robots.PRISMATIC).any()
        q[: n // 2, cont] = rng.choice([-1.0, 1.0], size=(n // 2, len(cont))) * 10 ** rng.uniform(
            4.5, 6, size=(n // 2, len(cont)))
        return Case(ch, q, far_goals(ch, rng, n), sample(ch, rng, n), kw | GOALS)
    if kind == "planar":
        ch = planar_chain()
        q = sample(ch, rng, n)
        return Case(ch, q, far_goals(ch, rng, n), sample(ch, rng, n), kw | dict(center_joints_weight=0.1))
    if kind == "dual_arm":
        ch = robots.torso_dual_arm()
        q = sample(ch, rng, n)
        return Case(ch, q, far_goals(ch, rng, n), sample(ch, rng, n), kw)
    raise ValueError(kind)


# (kind, step sizes, samples): every step size of the issue once or more; batch sizes off the multiples of 64
# (every robot at a step the fast kernels serve, <= 1e-2, and at one the literal kernels serve for every flavour)
CASES = [("panda_far", 1e-12, 21), ("panda_goals", 1e-8, 17), ("panda_far", 1e-4, 33), ("panda_near_pi", 1e-4, 19),
         ("ur5_limits", 1e-3, 23), ("ur5_limits", np.nextafter(1e-3, 1.0), 23), ("rr_axis", 1e-2, 31),
         ("random", 1e-4, 19), ("random", 1e-2, 17), ("random", 3e-2, 17), ("planar", 1e-4, 29), ("planar", 0.1, 29),
         ("panda_goals", 0.3, 17), ("dual_arm", 1e-4, 13), ("dual_arm", 1e-2, 13), ("dual_arm", 0.3, 13),
         ("panda_near_pi", 1.0, 17), ("random", 1.0, 13), ("rr_axis", 0.1, 65)]


@pytest.mark.parametrize("kind,h,n", CASES, ids=[f"{k}-{h:.17g}" for k, h, _ in CASES])
def test_step_stages(kind, h, n):
    check(f"{kind}-{h:.17g}", make_case(kind, h, n))


@pytest.mark.parametrize("scales", [(0.0, 0.5), (1.0, 0.0)], ids=["rotation_only", "position_only"])
@pytest.mark.parametrize("h", [1e-4, 0.3])
def test_step_with_one_pose_term(scales, h):
    """position_scale = 0 or rotation_scale = 0: the dropped term is neither in the cost nor in the probes"""
    rng = np.random.default_rng(21)
    ch = robots.panda()
    n = 19
    case = Case(ch, sample(ch, rng, n), far_goals(ch, rng, n), sample(ch, rng, n),
                dict(gd_step_size=h, position_scale=scales[0], rotation_scale=scales[1]))
    check(f"scales {scales} h {h}", case)


def test_step_with_zero_gradient():
    """both pose terms off and no joint goal: the cost is 0 everywhere, the gradient exactly 0, cost_diff 0 and
    joint_diff = 0 / 0 is set to 0 -- the update leaves q where it is (clamped)"""
    rng = np.random.default_rng(22)
    ch = robots.ur5()
    n = 17
    q = sample(ch, rng, n)
    case = Case(ch, q, far_goals(ch, rng, n), q, dict(position_scale=0.0, rotation_scale=0.0))
    check("zero gradient", case, min_share=0.0)
    for fl in FLAVOURS:
        s = solver(ch, fl)
        try:
            local, _, lc, _, G, _ = s.gd_step(pk.default_params(**case.kw), case.goal, q, q, q, np.zeros(n),
                                              np.zeros(n))
        finally:
            s.close()
        np.testing.assert_array_equal(G, 0.0)
        np.testing.assert_array_equal(local, q)
        np.testing.assert_array_equal(lc, 0.0)


def eigen_goal_norm2(gq):
    """|quaternion|^2 of the goal as the kernels re-derive it (toRotationMatrix, then back), in doubles"""
    return float(sum(x * x for x in H.goal_quat(gq)))


@pytest.mark.parametrize("h", [1e-4, 0.3])
def test_step_with_goal_quaternions_off_unit_norm(h):
    """goal quaternions whose re-derived norm^2 is 1 -+ 3e-9 .. 1e-6: both sides of make_probe_base's 1e-8 switch
    (1 / n2 as 2 - n2, or a divide).  The library takes a non-unit goal as upstream does -- Eigen's toRotationMatrix
    and back (pik_math.hpp make_goal; hp_reference.goal_quat) -- not as the normalised quaternion"""
    rng = np.random.default_rng(23)
    ch = robots.panda()
    n = 24
    q = sample(ch, rng, n)
    goal = far_goals(ch, rng, n)
    scale = np.array([1 + 3e-9, 1 - 3e-9, 1 + 3e-8, 1 - 3e-8, 1 + 1e-6, 1 - 1e-6] * 4)
    goal[:, 3:] *= scale[:, None]
    dev = np.array([1 - eigen_goal_norm2(g[3:]) for g in goal])
    assert (np.abs(dev) < 1e-8).sum() >= 4 and (np.abs(dev) > 1e-8).sum() >= 8, dev
    check(f"off-unit goals h {h}", Case(ch, q, goal, sample(ch, rng, n), dict(gd_step_size=h)))


@pytest.mark.parametrize("h", [np.nextafter(1e-2, 1.0), 0.3])
def test_large_steps_take_the_literal_kernels(h):
    """a fast handle serves gd_step_size > 1e-2 by the literal kernels: whole solves and steps bit-identical to the
    exact handle's (Panda, memetic and local mode)"""
    ch = robots.panda()
    rng = np.random.default_rng(24)
    q = sample(ch, rng, 40)
    seed = sample(ch, rng, 40)
    fast, exact = solver(ch, "fast"), solver(ch, "exact")
    try:
        goal = exact.fk(q)
        for kw in (dict(memetic_population_size=24, memetic_max_generations=8), dict(mode=1, gd_max_iters=30)):
            p = pk.default_params(gd_step_size=h, **kw)
            assert fast.kernel_name(p) == exact.kernel_name(p), (fast.kernel_name(p), exact.kernel_name(p))
            for x, y, w in zip(fast.solve_batch(p, goal, seed, rng_seed=3), exact.solve_batch(p, goal, seed, rng_seed=3),
                               ("solution", "status", "cost", "stats")):
                np.testing.assert_array_equal(x, y, err_msg=f"h {h} {kw} {w}")
        c0 = exact.cost(p, goal, seed, q)[0]
        for x, y in zip(fast.gd_step(p, goal, seed, q, q, c0, c0), exact.gd_step(p, goal, seed, q, q, c0, c0)):
            np.testing.assert_array_equal(x, y)
    finally:
        fast.close()
        exact.close()
