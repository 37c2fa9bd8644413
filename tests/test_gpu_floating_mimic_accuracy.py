"""Chains with a floating joint and chains with mimic joints -- which the exact (literal) kernels serve in every
library, exact (the default), exact=False and strict=True -- against the high-precision reference
(tests/hp_reference.py): Solver.fk, Solver.cost, Solver.gd_step stage by stage and whole solves, within bounds from
error analysis.  The bounds start from those of tests/test_gpu_fk_accuracy.py and tests/test_gpu_step_accuracy.py
(u = 2^-53, a = 8 (D + 2) u + sum_j f_j the error of a chain product of D steps, R = hp_reference.reach()).

  mimic joints   one more step each (D counts them).  The value fl(m q + o) is off by <= 2 u (|m q| + |o|): an angle,
                 among the f_j, for a revolute mimic joint; a length, added to the position bound, for a prismatic one.
                 The frames stay rotations, so everything else is as for the other chains (hp_reference.pose_errors).
  floating step  Translation(v0 v1 v2) * toRotationMatrix(w = v6, v3, v4, v5), not normalised: with s the quaternion's
                 norm the matrix is s^2 R' + (1 - s^2) I, a normal matrix of 2-norm kappa = max(1, 2 s^2 - 1) (<= 7
                 within the limits).  Its entries 1 - (2yy + 2zz), 2xy - 2wz, ... carry <= (6 s^2 + 1) u <= 7 u kappa,
                 the origin product and the product with the frame 3 u each: two steps' worth, and its seven
                 variables count as seven steps of D.
  position       <= a R: every translation behind a floating step, and every rounding error in front of it, is
                 multiplied by kappa on its way to the tip -- reach() counts those translations kappa times
                 (hp_reference.scaling is the product of the kappas along the path).
  matrix         e_M = a kappa per entry of the tip frame, which is no rotation: the quaternion Eigen's conversion
                 takes from it is not unit and depends on the branch taken, so Solver.fk is compared component by
                 component (hp_reference.component_errors), sign included.
  quaternion     In every branch of the conversion the square root's argument A is >= 1 for every such matrix
                 (trace branch: trace + 1 > 1; otherwise 2 m_ii - trace + 1 >= 1 - trace / 3 >= 1), so t = sqrt(A)
                 is off by <= dA / 2 <= 1.5 e_M and the divisions by t are well conditioned: the component t / 2 is
                 off by <= 0.75 e_M, a component (m_ab +- m_ba) / (2 t) by <= e_M + 1.5 m e_M, m the largest entry;
                 e_q = 2 (1 + m) e_M + 4 u (1 + m)^2 covers both and the roundings of the conversion itself.
  branch         The conversion decides by trace > 0, m_11 > m_00 and m_22 > m_ii.  Where the reference's margin of
                 a decision (hp_reference.branch_decisions) is <= 3 e_M the kernels may decide the other way: the
                 value must then match the reference under the branch that outcome leads to, within the same bound.
                 Either is accepted, nothing is excluded.
  angle          angularDistance depends on neither norm.  An error d of the 4-vector q turns it by <= |d| / |q|, the
                 angle by twice that: e_a = 4 e_q / |q_tip| + 4 e_q(goal) / |q_goal| + EXTRACT, the norms from the
                 reference per sample (Eigen's quaternion of any of these matrices has a component >= 1/2).  The
                 goal's matrix is built from the given doubles (entries off by <= 7 u kappa_goal) and converted the
                 same way.
  cost, step     as in tests/test_gpu_step_accuracy.py with these e_p and e_a: every probe is the literal difference
                 of two costs (e_g = e_c(+) + e_c(-) + u |g_j|).

The frames of a floating chain scale with s^2, so goals taken from its own frames are up to 7 times farther out than
the arm reaches: costs reach 1e2, and a bound is typically 1e-13 .. 1e-12 of which roundings use a few per cent (the
per-step 8 u is a worst case that the three-term dot products never meet together; DESIGN.md section 3 records the
measured fractions, those of the CPU oracle included).

Every batch holds, besides samples drawn uniformly inside the limits (at least half), the edges of `edge_samples`:
unit base quaternions, all four components at +-1 (s^2 = 4), |q| from 1e-8 down to exactly 0 (the identity, trace
branch), a component at a limit and nextafter inside it, translations at their limits, and samples solved by
bisection on the reference to sit on a branch decision of the tip frame (the trace within 1e-9 of 0, down to what
the doubles resolve, 1e-15 and below; likewise the two largest diagonal entries tied while the trace is < 0).
"""
import itertools
import zlib

import numpy as np
import pytest

import pick_ik_amd as pk
from pick_ik_amd import robots
from tests import hp_reference as H
from tests import test_gpu_fk_accuracy as A
from tests import test_gpu_step_accuracy as S
from tests.test_gpu_floating import with_floating_joint
from tests.test_gpu_fuzz import random_chain
from tests.test_mimic_cpu import prismatic_and_two_in_a_row, with_mimic

pytestmark = pytest.mark.gpu

U = H.EPS
FLAVOURS = tuple(A.FLAVOURS)
GOALS = dict(center_joints_weight=0.05, avoid_joint_limits_weight=0.1, minimal_displacement_weight=0.01)


# ---------------------------------------------------------------------------------------------------------------
# chains
# ---------------------------------------------------------------------------------------------------------------
def generated_floating(where, others):
    """tests/test_gpu_floating.py with_floating_joint on a generated chain of `others` joints, the first seed that
    puts the floating joint in the middle of them / behind the last"""
    for k in itertools.count():
        rng = np.random.default_rng(0xF10A7 + 1000 * others + k)
        ch = with_floating_joint(rng, random_chain(rng, others))
        at = int(np.flatnonzero(ch.joint_type == robots.FLOATING_TX)[0])
        if (where == "end" and at == others) or (where == "middle" and 0 < at < others):
            return ch


def two_tip_floating():
    """two three-joint arms on one floating base: both tip paths start with the same seven variables"""
    base = robots.on_floating_base(robots.rr(), origin=(0.05, 0.1, 0.2, 0.3, -0.2, 0.1), reach=0.4)

    def arm(side, first):
        origins = [[0.0, 0.15 * side, 0.1, 0.4 * side, 0, 0], [0.25, 0, 0, 0, 0.3, 0], [0.2, 0, 0, 0.2, 0, 0]]
        axes = [[0, 0, 1], [0, 1, 0], [0.2, 1, 0]]
        tip = [0.1, 0, 0.05, 0, 0, 0.5 * side]
        return (list(range(7)) + [first, first + 1, first + 2], np.concatenate([base.origin_xyz_rpy[:7], origins]),
                np.concatenate([base.axis[:7], axes]), list(robots.FLOATING) + [0, 0, 0], tip)

    lim = [2.0, 1.5, 2.5] * 2
    return robots.multi_chain("two_tip_floating", [arm(1.0, 7), arm(-1.0, 10)], list(base.qmin[:7]) + [-x for x in lim],
                              list(base.qmax[:7]) + lim, [1.0] * 13)


def revolute_mimic():
    return with_mimic(None, robots.panda(), 3, 1, -0.6, 0.2)[0]


CHAINS = {"floating_panda": robots.floating_panda, "floating_middle": lambda: generated_floating("middle", 4),
          "floating_end": lambda: generated_floating("end", 3), "mimic_revolute": revolute_mimic,
          "mimic_prismatic": lambda: prismatic_and_two_in_a_row()[0], "two_tip_floating": two_tip_floating}
_chains = {}


def chain(name):
    if name not in _chains:
        _chains[name] = CHAINS[name]()
    return _chains[name]


def floating_blocks(ch):
    """the variables (seven each) of the chain's floating joints"""
    out = []
    for p in H.paths(ch):
        for j, t in enumerate(p.joint_type):
            v = [int(x) for x in p.variable[j:j + 7]]
            if int(t) == robots.FLOATING_TX and v not in out:
                out.append(v)
    return out


# ---------------------------------------------------------------------------------------------------------------
# samples
# ---------------------------------------------------------------------------------------------------------------
def uniform(ch, rng, n):
    """uniform inside the limits (the limits of an unbounded generated variable too: +-1 for a quaternion variable)"""
    return rng.uniform(ch.qmin, ch.qmax, size=(n, ch.dof))


def tip_matrix(ch, x, tip=0):
    return H.fk(ch, x)[tip][1]


def bisect(ch, x, v, f, lo, hi, target):
    """x with variable v moved inside [lo, hi], where f(tip matrix) changes sign, until |f| <= target (doubles)"""
    x = x.copy()

    def at(c):
        x[v] = c
        return f(tip_matrix(ch, x))

    flo = at(lo)
    for _ in range(80):
        mid = 0.5 * (lo + hi)
        if mid in (lo, hi):
            break
        fm = at(mid)
        if abs(fm) <= target:
            lo = mid
            break
        if (fm > 0) == (flo > 0):
            lo, flo = mid, fm
        else:
            hi = mid
    x[v] = lo
    return x


def trace(R):
    return R[0][0] + R[1][1] + R[2][2]


def on_a_decision(ch, rng, block, kind, target):
    """a uniform sample with one base-quaternion variable solved so that the tip frame sits on a branch decision of
    Eigen's conversion: kind "trace": |trace| <= target; "diagonal": the two largest diagonal entries within target
    of each other, the trace < 0"""
    grid = np.linspace(-1.0, 1.0, 9)
    while True:
        x = uniform(ch, rng, 1)[0]
        v = block[3 + int(rng.integers(4))]
        rows = []
        for c in grid:
            y = x.copy()
            y[v] = c
            R = tip_matrix(ch, y)
            rows.append(([R[0][0], R[1][1], R[2][2]], trace(R)))
        for k in range(len(grid) - 1):
            (d0, t0), (d1, t1) = rows[k], rows[k + 1]
            if kind == "trace":
                if (t0 > 0) != (t1 > 0):
                    return bisect(ch, x, v, trace, grid[k], grid[k + 1], target)
                continue
            order = sorted(range(3), key=lambda i: d0[i])
            a, b = order[2], order[1]  # the two largest at the left end: swapped at the right end, the third below
            if t0 < 0 and t1 < 0 and d1[b] > d1[a] and d1[order[0]] < d1[a] and d0[order[0]] < d0[b]:
                y = bisect(ch, x, v, lambda R: R[a][a] - R[b][b], grid[k], grid[k + 1], target)
                R = tip_matrix(ch, y)
                if trace(R) < 0 and R[order[0]][order[0]] < min(R[a][a], R[b][b]):
                    return y


def edge_samples(ch, rng, n):
    """n edge samples (see the module docstring); for a chain without a floating joint: variables at their limits
    and nextafter inside them"""
    q = uniform(ch, rng, n)
    blocks = floating_blocks(ch)
    if not blocks:
        for i in range(n):
            v = int(rng.integers(ch.dof))
            lim = (ch.qmin, ch.qmax)[i % 2]
            q[i, v] = lim[v] if i % 4 < 2 else np.nextafter(lim[v], 0.0)
            if i % 5 == 4:
                q[i] = lim
        return q
    b = blocks[0]
    quat = b[3:]
    tiny = itertools.cycle([1e-8, 0.0, 1e-12, 1e-30, 1e-160, 1e-300])
    # (the first of each kind inside the matrix error bound, so that the smallest batch has such a sample too)
    targets = {"trace": itertools.cycle([1e-15, 1e-10, 1e-13, 1e-9, 1e-14, 1e-11]),
               "diagonal": itertools.cycle([1e-14, 1e-11, 1e-15, 1e-9, 1e-13, 1e-10])}
    for i in range(n):
        kind = i % 9
        if kind == 0:    # a unit base quaternion: every frame a rotation
            q[i, quat] /= np.linalg.norm(q[i, quat])
        elif kind == 1:  # s^2 = 4, the largest scaling
            q[i, quat] = rng.choice([-1.0, 1.0], size=4)
        elif kind == 2:  # |q| -> 0: the identity
            s = next(tiny)
            q[i, quat] = s * rng.choice([-1.0, 1.0], size=4) * rng.uniform(0.1, 0.5, size=4)
        elif kind == 3:  # one component at a limit
            v = quat[int(rng.integers(4))]
            q[i, v] = (ch.qmin, ch.qmax)[i % 2][v]
        elif kind == 4:  # ... and nextafter inside it
            v = quat[int(rng.integers(4))]
            q[i, v] = np.nextafter((ch.qmin, ch.qmax)[i % 2][v], 0.0)
        elif kind == 5:  # translations at their limits
            q[i, b[:3]] = np.where(rng.uniform(size=3) < 0.5, ch.qmin[b[:3]], ch.qmax[b[:3]])
        elif kind == 6:
            q[i] = on_a_decision(ch, rng, b, "trace", next(targets["trace"]))
        elif kind == 7:
            q[i] = on_a_decision(ch, rng, b, "diagonal", next(targets["diagonal"]))
        else:            # exactly 0: the frame behind it is the frame in front of it
            q[i, quat] = 0.0
    return q


_samples = {}


def samples(name, n):
    """the batch of a chain: n // 2 edge samples behind the uniform ones"""
    if (name, n) not in _samples:
        ch = chain(name)
        rng = np.random.default_rng(zlib.crc32(f"{name} {n}".encode()))
        q = np.concatenate([uniform(ch, rng, n - n // 2), edge_samples(ch, rng, n // 2)])
        q.setflags(write=False)
        _samples[name, n] = q
    return _samples[name, n]


def as_goal(ch, pose):
    return np.asarray(pose).reshape(7 * len(getattr(ch, "tips", [None])))


def far_goals(ch, rng, n):
    """the exact frames of other uniform samples (behind a floating joint: no rotations, their quaternions not unit)"""
    return np.array([as_goal(ch, H.pose7(ch, x)) for x in uniform(ch, rng, n)])


def near_goals(ch, q, rng):
    """tests/test_gpu_fk_accuracy.py goals_around, per tip: 1e-12 .. 1e-2 away from the frame in position and in
    angle, near 180 degrees and near 2 pi / 3"""
    n_tips = len(getattr(ch, "tips", [None]))
    g = np.array([as_goal(ch, H.pose7(ch, x)) for x in q]).reshape(len(q), n_tips, 7)
    for k in range(n_tips):
        g[:, k] = A.goals_around_frames(g[:, k], rng)
    return g.reshape(len(q), 7 * n_tips)


# ---------------------------------------------------------------------------------------------------------------
# bounds (see the module docstring); every handle is served by the exact kernels: the flavour of the bounds is "exact"
# ---------------------------------------------------------------------------------------------------------------
def matrix_bound(ch, x):
    return A.fk_bounds(ch, x, "exact")[1] * H.scaling(ch, x)


def marginal(R, e_mat):
    """the branches that a decision within 3 e_M of its margin may lead to instead of the reference's"""
    return [other for margin, other in H.branch_decisions(R) if float(margin) <= 3 * e_mat]


def branch_choices(ch, x, frames):
    """per-tip branch lists to try: the reference's own (None) first, then what the marginal decisions allow"""
    e = matrix_bound(ch, x)
    return list(itertools.product(*[[None] + marginal(R, e) for _, R in frames]))


def literal_handle(ch, flavour):
    """the handle of a flavour; one made with exact=False is served by the exact kernels too"""
    s = A.solver(ch, flavour)
    if flavour == "fast":
        for kw in (dict(), dict(mode=1), dict(gd_step_size=1e-8)):
            name = s.kernel_name(pk.default_params(**kw))
            assert name.startswith("pik_exact::"), (ch.name, kw, name)
    return s


# ---------------------------------------------------------------------------------------------------------------
# FK
# ---------------------------------------------------------------------------------------------------------------
REF_FK = {}


def check_fk_components(name, n, flavours=FLAVOURS, handle=literal_handle):
    """position and every quaternion component (Eigen's sign) of a floating chain's tip frames"""
    ch, q = chain(name), samples(name, n)
    if (name, n) not in REF_FK:
        REF_FK[name, n] = [H.fk(ch, x) for x in q]
    frames = REF_FK[name, n]
    report = {}
    for fl in flavours:
        s = handle(ch, fl)
        try:
            got = s.fk(q).reshape(n, -1, 7)
        finally:
            s.close()
        worst = dict(p=0.0, q=0.0, other_branch=0, on_a_decision=0)
        for i in range(n):
            ep = A.fk_bounds(ch, q[i], "exact")[0]
            e_mat = matrix_bound(ch, q[i])
            for k, (t, R) in enumerate(frames[i]):
                eq = A.quat_bound(R, e_mat)
                alts = marginal(R, e_mat)
                worst["on_a_decision"] += bool(alts)
                errs = [H.component_errors([(t, R)], got[i, k], b)[0] for b in [None] + alts]
                dp, dq = errs[0][0], min(e[1] for e in errs)
                assert dp <= ep, (name, fl, i, k, "position", dp, ep, q[i].tolist())
                assert dq <= eq, (name, fl, i, k, "quaternion", [e[1] for e in errs], eq, alts, q[i].tolist())
                worst["other_branch"] += errs[0][1] > eq
                worst["p"], worst["q"] = max(worst["p"], dp / ep), max(worst["q"], dq / eq)
        report[fl] = {k: round(v, 3) for k, v in worst.items()}
    print(name, n, "fk", report)
    return report


FLOATING = ["floating_panda", "floating_middle", "floating_end", "two_tip_floating"]
MIMIC = ["mimic_revolute", "mimic_prismatic"]


@pytest.mark.parametrize("name,n", [(c, n) for c in FLOATING for n in (21, 65)])
def test_fk_floating(name, n):
    r = check_fk_components(name, n)
    assert all(v["on_a_decision"] >= 1 for v in r.values()), r  # (the samples built for it are there)


@pytest.mark.parametrize("name", MIMIC)
def test_fk_mimic(name):
    """the frames are rotations: position and angle as for every other chain, and the norm of the quaternion"""
    ch, q = chain(name), samples(name, 65)
    for fl in FLAVOURS:
        literal_handle(ch, fl).close()
    print(name, "fk", A.check_fk(ch, q, what=name))


# ---------------------------------------------------------------------------------------------------------------
# cost and verdict
# ---------------------------------------------------------------------------------------------------------------
COST_KW = dict(GOALS, cost_threshold=0.3, position_threshold=3e-3, orientation_threshold=3e-3, position_scale=1.0,
               rotation_scale=0.5)


def cost_case(name, n):
    ch, q = chain(name), samples(name, n)
    rng = np.random.default_rng(zlib.crc32(f"cost {name} {n}".encode()))
    goal = near_goals(ch, q, rng)
    goal[1::3] = far_goals(ch, rng, len(goal[1::3]))
    return ch, q, goal, uniform(ch, rng, n)


def matching_cost(ch, p, goal, seed, x, value, ref):
    """(the reference cost that `value` is within its bound of, the error as a fraction of the bound, whether that
    took another branch than the reference's own): the reference's own first, then the marginal branches"""
    first = None
    for branch in branch_choices(ch, x, ref.frames):
        r = ref if not any(branch) else H.cost(ch, p, goal, seed, x, branch=list(branch))
        e = S.cost_bound(ch, p, "exact", x, r)
        d = abs(value - float(r.cost))
        first = first or (d, e)
        if d <= e:
            return r, d / e if e > 0 else 0.0, any(branch)
    raise AssertionError(("cost", ch.name, value, float(ref.cost), first, x.tolist()))


def at_a_threshold(ch, p, x, r):
    """a distance or an angle of r = hp_reference.cost at x within its error of its threshold, or a joint goal
    within the cost's rounding of cost_threshold^2: where alone a verdict may differ from the reference's"""
    ep = A.fk_bounds(ch, x, "exact")[0]
    return (any(abs(float(lin) - p.position_threshold) <= ep for lin in r.lin)
            or any(abs(float(ang) - p.orientation_threshold) <= ea
                   for ang, ea in zip(r.ang, A.angle_bounds(ch, x, "exact", r)))
            or any(abs(float(v) * w * w - p.cost_threshold ** 2) <= 16 * U for w, v in r.goal_terms))


REF_COST = {}


def check_cost(name, n, flavours=FLAVOURS, handle=literal_handle):
    ch, q, goal, seed = cost_case(name, n)
    p = pk.default_params(**COST_KW)
    if (name, n) not in REF_COST:
        REF_COST[name, n] = [H.cost(ch, p, goal[i], seed[i], q[i]) for i in range(n)]
    refs = REF_COST[name, n]
    assert len({r.solution for r in refs}) == 2, "both verdicts among the samples"
    neg = goal.reshape(n, -1, 7).copy()
    neg[:, :, 3:] *= -1.0
    report = {}
    for fl in flavours:
        s = handle(ch, fl)
        try:
            c, sol = s.cost(p, goal, seed, q)
            c2, sol2 = s.cost(p, neg.reshape(n, -1), seed, q)
        finally:
            s.close()
        np.testing.assert_array_equal(c, c2, err_msg=f"{name} {fl}: goal quaternion -q")
        np.testing.assert_array_equal(sol, sol2, err_msg=f"{name} {fl}: goal quaternion -q")
        worst, other = 0.0, 0
        for i in range(n):
            r, f, alt = matching_cost(ch, p, goal[i], seed[i], q[i], c[i], refs[i])
            worst, other = max(worst, f), other + alt
            if bool(sol[i]) != r.solution:
                assert at_a_threshold(ch, p, q[i], r), (name, fl, i, bool(sol[i]), [float(x) for x in r.lin + r.ang])
        report[fl] = dict(cost=round(worst, 3), other_branch=other)
    print(name, n, "cost", report)
    return report


@pytest.mark.parametrize("name,n", [(c, n) for c, n in zip(FLOATING + MIMIC, (33, 21, 65, 21, 33, 65))])
def test_cost_and_verdict(name, n):
    check_cost(name, n)


# ---------------------------------------------------------------------------------------------------------------
# step stages
# ---------------------------------------------------------------------------------------------------------------
def step_case(name, h, n):
    """tests/test_gpu_step_accuracy.py Case: the chain's batch, far goals, joint goals on for every other case; a
    quarter of the samples with quaternion variables (a master variable for a mimic chain) within h of a limit, so
    that the probes leave the limits and the update clamps"""
    ch = chain(name)
    q = samples(name, n).copy()
    rng = np.random.default_rng(zlib.crc32(f"step {name} {h!r} {n}".encode()))
    blocks = floating_blocks(ch)
    vs = blocks[0][3:] if blocks else sorted({int(m.master_variable) for m in ch.mimic})
    for i in range(0, n - n // 2, 4):
        for v in vs:
            if rng.uniform() < 0.5:
                lim = (ch.qmin, ch.qmax)[int(rng.integers(2))][v]
                q[i, v] = lim - np.sign(lim) * h * rng.uniform(0, 1)
    kw = dict(gd_step_size=h) | (GOALS if h != 1e-4 else {})
    return S.Case(ch, q, far_goals(ch, rng, n), uniform(ch, rng, n), kw, literal=True)


STEP_CASES = [(c, h, n) for c, sizes in (("floating_panda", (21, 33, 21)), ("floating_middle", (33, 21, 21)),
                                         ("floating_end", (21, 21, 65)), ("two_tip_floating", (21, 21, 21)),
                                         ("mimic_revolute", (21, 65, 33)), ("mimic_prismatic", (65, 33, 21)))
              for h, n in zip((1e-8, 1e-4, 0.3), sizes)]


@pytest.mark.parametrize("name,h,n", STEP_CASES, ids=[f"{c}-{h:g}" for c, h, _ in STEP_CASES])
def test_step_stages(name, h, n):
    S.check(f"{name}-{h:g}-{n}", step_case(name, h, n))


# ---------------------------------------------------------------------------------------------------------------
# whole solves
# ---------------------------------------------------------------------------------------------------------------
SOLVES = {"local": dict(mode=1, gd_max_iters=60),
          "memetic": dict(memetic_population_size=16, memetic_max_generations=10)}
SOLVE_SEED = {("floating_panda", "local"): 1, ("floating_panda", "memetic"): 1, ("mimic_revolute", "local"): 1,
              ("mimic_revolute", "memetic"): 1}  # (chosen with the oracle: at least one problem succeeds)


def solve_case(name, B=32):
    """goals: frames of the chain at unit base quaternions (rotations, reachable), a step away from the seeds"""
    ch = chain(name)
    rng = np.random.default_rng(zlib.crc32(f"solve {name}".encode()))
    seed = uniform(ch, rng, B)
    for b in floating_blocks(ch):
        seed[:, b[3:]] /= np.linalg.norm(seed[:, b[3:]], axis=1, keepdims=True)
    target = np.clip(seed + rng.normal(0, 0.05, size=seed.shape), ch.qmin, ch.qmax)
    for b in floating_blocks(ch):
        target[:, b[3:]] /= np.linalg.norm(target[:, b[3:]], axis=1, keepdims=True)
    goal = np.array([as_goal(ch, H.pose7(ch, x)) for x in target])
    return ch, goal, seed


def check_solves(name, how, flavours=FLAVOURS, handle=literal_handle):
    ch, goal, seed = solve_case(name)
    p = pk.default_params(**SOLVES[how])
    report = {}
    for fl in flavours:
        s = handle(ch, fl)
        try:
            sol, status, cost, _ = s.solve_batch(p, goal, seed, rng_seed=SOLVE_SEED[name, how])
        finally:
            s.close()
        worst = 0.0
        for i in range(len(goal)):
            ref = H.cost(ch, p, goal[i], seed[i], sol[i])
            r, f, _ = matching_cost(ch, p, goal[i], seed[i], sol[i], cost[i], ref)
            worst = max(worst, f)
            if status[i] == 1 and not r.solution:  # SUCCESS: a solution for the reference too, or at a threshold
                assert at_a_threshold(ch, p, sol[i], r), (name, how, fl, i, [float(x) for x in r.lin + r.ang])
        assert (status == 1).sum() >= 1, (name, how, fl, status)
        report[fl] = dict(cost=round(worst, 3), solved=f"{int((status == 1).sum())}/{len(goal)}")
    print(name, how, report)
    return report


@pytest.mark.parametrize("how", list(SOLVES))
@pytest.mark.parametrize("name", ["floating_panda", "mimic_revolute"])
def test_whole_solves(name, how):
    check_solves(name, how)
