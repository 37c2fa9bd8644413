"""High-precision reference of the forward kinematics and the cost function (test-only code).

Everything here is computed with mpmath at PREC bits (128; double rounding is 53) from the chain description of
pick_ik_amd.robots (`origin_xyz_rpy`, `axis`, `joint_type`, `tip_xyz_rpy`; `MultiChain.tips` for several tip
frames), independently of the library and of the CPU oracle: none of their arithmetic is reused, so an error that the
kernels and the oracle share (a sine, an arctangent, a quaternion extraction) shows up against this module.

  fk(chain, q)                        URDF origins (R = Rz(yaw) Ry(pitch) Rx(roll)), a Rodrigues rotation about the
                                      normalised axis for revolute / continuous joints, a translation along it for
                                      prismatic joints, planar joints as x / y translations + a rotation about z
                                      (MoveIt's PlanarJointModel); the exact position and rotation matrix per tip
  angular_distance(R, goal_quat)      Eigen's angularDistance, 2 atan2(|vec|, |w|) of the relative quaternion
  cost(chain, params, goal, seed, q)  the upstream make_cost_fn (pose cost src/goal.cpp:51-78, joint goals :91-144,
                                      weight^2 composition :163-203) and the solution test (frame tests
                                      src/goal.cpp:27-36, joint goals against cost_threshold^2)

Floating and mimic joints are not modelled: chains with them stay with the oracle (oracle/pik_oracle.c), whose
literal chain product the exact flavours match bit for bit.

  step(chain, params, goal, seed, q)  step() of src/ik_gradient.cpp:24-94 taken literally, every cost by `cost`: the
                                      raw and normalised gradient, the line search and the clamped update (`Step`)

The inputs are doubles and are taken as exact, the goal quaternion included: it goes through Eigen's
toRotationMatrix and back as upstream's does (`goal_quat`), so a goal quaternion off unit norm gives upstream's
angle, not that of the normalised quaternion.
"""
from __future__ import annotations

import dataclasses
import math

import mpmath
import numpy as np

from pick_ik_amd import robots

PREC = 128
M = mpmath.MPContext()
M.prec = PREC
EPS = 2.0 ** -53  # unit roundoff of binary64


def mpf(x):
    return M.mpf(float(x))


def _matmul(A, B):
    return [[A[i][0] * B[0][j] + A[i][1] * B[1][j] + A[i][2] * B[2][j] for j in range(3)] for i in range(3)]


def _matvec(A, v):
    return [A[i][0] * v[0] + A[i][1] * v[1] + A[i][2] * v[2] for i in range(3)]


def _ident():
    return [[M.mpf(1) if i == j else M.mpf(0) for j in range(3)] for i in range(3)]


def rpy_matrix(r, p, y):
    """urdf::Rotation::setFromRPY: Rz(yaw) Ry(pitch) Rx(roll)"""
    cr, sr, cp, sp, cy, sy = M.cos(r), M.sin(r), M.cos(p), M.sin(p), M.cos(y), M.sin(y)
    return [[cy * cp, cy * sp * sr - sy * cr, cy * sp * cr + sy * sr],
            [sy * cp, sy * sp * sr + cy * cr, sy * sp * cr - cy * sr],
            [-sp, cp * sr, cp * cr]]


def rodrigues(n, th):
    """rotation by th about the unit axis n"""
    c, s = M.cos(th), M.sin(th)
    v = 1 - c
    x, y, z = n
    return [[c + v * x * x, v * x * y - s * z, v * x * z + s * y],
            [v * x * y + s * z, c + v * y * y, v * y * z - s * x],
            [v * x * z - s * y, v * y * z + s * x, c + v * z * z]]


@dataclasses.dataclass
class _Path:
    variable: np.ndarray
    origin_xyz_rpy: np.ndarray
    axis: np.ndarray
    joint_type: np.ndarray
    tip_xyz_rpy: np.ndarray


def paths(chain):
    """the serial paths of a chain (one per tip frame)"""
    if getattr(chain, "mimic", ()):
        raise NotImplementedError("mimic joints: compare with the oracle")
    if hasattr(chain, "tips"):
        ps = [_Path(t.variable, t.origin_xyz_rpy, t.axis, t.joint_type, t.tip_xyz_rpy) for t in chain.tips]
    else:
        ps = [_Path(np.arange(chain.dof), chain.origin_xyz_rpy, chain.axis, chain.joint_type, chain.tip_xyz_rpy)]
    for p in ps:
        if any(int(t) in robots.FLOATING for t in p.joint_type):
            raise NotImplementedError("floating joints: compare with the oracle")
    return ps


def _origin(xyz_rpy):
    return rpy_matrix(*(mpf(v) for v in xyz_rpy[3:])), [mpf(v) for v in xyz_rpy[:3]]


def _fk_path(p, q):
    R, t = _ident(), [M.mpf(0)] * 3
    for j in range(len(p.variable)):
        jt = int(p.joint_type[j])
        v = mpf(q[int(p.variable[j])])
        if jt in (robots.PLANAR_X, robots.PLANAR_Y, robots.PLANAR_THETA):
            k = jt - robots.PLANAR_X  # x, y: translations along the joint frame's x / y; theta: about z
            if k == 0:
                Ro, to = _origin(p.origin_xyz_rpy[j])
                t = [a + b for a, b in zip(t, _matvec(R, to))]
                R = _matmul(R, Ro)
            n = [M.mpf(int(i == k)) for i in range(3)] if k < 2 else [M.mpf(0), M.mpf(0), M.mpf(1)]
            jt = robots.REVOLUTE if k == 2 else robots.PRISMATIC
        else:
            Ro, to = _origin(p.origin_xyz_rpy[j])
            t = [a + b for a, b in zip(t, _matvec(R, to))]
            R = _matmul(R, Ro)
            a = [mpf(x) for x in p.axis[j]]
            nn = M.sqrt(a[0] ** 2 + a[1] ** 2 + a[2] ** 2)
            n = [x / nn for x in a]
        if jt == robots.PRISMATIC:
            t = [a + b for a, b in zip(t, _matvec(R, [x * v for x in n]))]
        else:
            R = _matmul(R, rodrigues(n, v))
    Ro, to = _origin(p.tip_xyz_rpy)
    t = [a + b for a, b in zip(t, _matvec(R, to))]
    return t, _matmul(R, Ro)


def fk(chain, q):
    """[(position[3], rotation[3][3])] per tip frame, as mpmath numbers"""
    return [_fk_path(p, q) for p in paths(chain)]


def matrix_to_quat(R):
    """the unit quaternion (w, x, y, z) of an exact rotation matrix, w >= 0"""
    tr = R[0][0] + R[1][1] + R[2][2]
    cands = [tr, R[0][0], R[1][1], R[2][2]]
    k = max(range(4), key=lambda i: cands[i])
    if k == 0:
        s = M.sqrt(tr + 1) * 2
        q = [s / 4, (R[2][1] - R[1][2]) / s, (R[0][2] - R[2][0]) / s, (R[1][0] - R[0][1]) / s]
    elif k == 1:
        s = M.sqrt(1 + R[0][0] - R[1][1] - R[2][2]) * 2
        q = [(R[2][1] - R[1][2]) / s, s / 4, (R[0][1] + R[1][0]) / s, (R[0][2] + R[2][0]) / s]
    elif k == 2:
        s = M.sqrt(1 + R[1][1] - R[0][0] - R[2][2]) * 2
        q = [(R[0][2] - R[2][0]) / s, (R[0][1] + R[1][0]) / s, s / 4, (R[1][2] + R[2][1]) / s]
    else:
        s = M.sqrt(1 + R[2][2] - R[0][0] - R[1][1]) * 2
        q = [(R[1][0] - R[0][1]) / s, (R[0][2] + R[2][0]) / s, (R[1][2] + R[2][1]) / s, s / 4]
    return [-x for x in q] if q[0] < 0 else q


def quat_mul(a, b):
    aw, ax, ay, az = a
    bw, bx, by, bz = b
    return [aw * bw - ax * bx - ay * by - az * bz, aw * bx + ax * bw + ay * bz - az * by,
            aw * by + ay * bw + az * bx - ax * bz, aw * bz + az * bw + ax * by - ay * bx]


def unit(qd):
    q = [mpf(x) for x in qd]
    n = M.sqrt(sum(x * x for x in q))
    return [x / n for x in q]


def quat_angle(qa, qb):
    """the rotation angle of qa * conj(qb) (Eigen angularDistance: 2 atan2(|vec|, |w|)), in [0, pi]"""
    d = quat_mul(qa, [qb[0], -qb[1], -qb[2], -qb[3]])
    return 2 * M.atan2(M.sqrt(d[1] ** 2 + d[2] ** 2 + d[3] ** 2), abs(d[0]))


def goal_quat(gq):
    """the goal quaternion as upstream sees it: tf2::fromMsg builds the goal frame's matrix with Eigen's
    toRotationMatrix, which does not normalise (a quaternion of norm s gives s^2 R + (1 - s^2) I), and
    angular_distance re-derives a quaternion from that matrix (src/goal.cpp:22-23) by Eigen's branches (the trace
    when it is > 0, else the largest diagonal entry) -- not a multiple of the given one unless it is unit"""
    w, x, y, z = (mpf(v) for v in gq)
    R = [[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
         [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
         [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]]
    tr = R[0][0] + R[1][1] + R[2][2]
    if tr > 0:
        t = M.sqrt(tr + 1)
        return [t / 2, (R[2][1] - R[1][2]) / (2 * t), (R[0][2] - R[2][0]) / (2 * t), (R[1][0] - R[0][1]) / (2 * t)]
    i = 0
    if R[1][1] > R[0][0]:
        i = 1
    if R[2][2] > R[i][i]:
        i = 2
    j, k = (i + 1) % 3, (i + 2) % 3
    t = M.sqrt(R[i][i] - R[j][j] - R[k][k] + 1)
    v = [M.mpf(0)] * 3
    v[i] = t / 2
    v[j] = (R[j][i] + R[i][j]) / (2 * t)
    v[k] = (R[k][i] + R[i][k]) / (2 * t)
    return [(R[k][j] - R[j][k]) / (2 * t)] + v


def angular_distance(R, gq):
    """Eigen angularDistance between the exact frame R and the goal quaternion (w, x, y, z) as upstream takes it
    (`goal_quat`); angularDistance itself does not depend on the norm of either quaternion"""
    return quat_angle(matrix_to_quat(R), goal_quat(gq))


def linear_distance(t, goal_t):
    return M.sqrt(sum((a - mpf(b)) ** 2 for a, b in zip(t, goal_t)))


def pose_cost(lin, ang, position_scale, rotation_scale):
    """make_pose_cost_fn, src/goal.cpp:51-78: a term is dropped when its scale is <= 0"""
    c = M.mpf(0)
    if position_scale > 0:
        c += (lin * mpf(position_scale)) ** 2
    if rotation_scale > 0:
        c += (ang * mpf(rotation_scale)) ** 2
    return c


def variables(chain):
    """Robot::from, src/robot.cpp:44-85: (bounded, mid, half_span, minimal displacement factor) per variable"""
    d = chain.dof
    lo, hi = [mpf(x) for x in chain.qmin], [mpf(x) for x in chain.qmax]
    rcp = [1 / mpf(v) if v > 0 else M.mpf(0) for v in chain.vmax]
    div = sum(rcp)
    out = []
    for j in range(d):
        b = int(chain.bounded[j]) != 0
        out.append((b, (lo[j] + hi[j]) / 2, (hi[j] - lo[j]) / 2 if b else +M.pi,
                    rcp[j] / div if div > 0 else M.mpf(1) / d))
    return out


def joint_goal_terms(chain, params, seed, q):
    """[(weight, unweighted cost)] of the enabled joint goals, in the plugin's order (src/pick_ik_plugin.cpp:118-129)"""
    var = variables(chain)
    qq, sd = [mpf(x) for x in q], [mpf(x) for x in seed]
    out = []
    if params.center_joints_weight > 0:  # src/goal.cpp:91-108
        out.append((params.center_joints_weight,
                    sum(((qq[i] - m) * f) ** 2 for i, (b, m, _, f) in enumerate(var) if b)))
    if params.avoid_joint_limits_weight > 0:  # :110-129
        out.append((params.avoid_joint_limits_weight,
                    sum((max(M.mpf(0), abs(qq[i] - m) * 2 - h) * f) ** 2 for i, (b, m, h, f) in enumerate(var) if b)))
    if params.minimal_displacement_weight > 0:  # :131-144
        out.append((params.minimal_displacement_weight, sum(((qq[i] - sd[i]) * var[i][3]) ** 2 for i in range(len(var)))))
    return out


@dataclasses.dataclass
class Cost:
    cost: object        # mpf: cost_fn
    solution: bool      # solution_fn
    lin: list           # per tip: |goal - frame| (mpf)
    ang: list           # per tip: angular distance (mpf)
    goal_terms: list    # [(weight, unweighted cost)] of the joint goals


def cost(chain, params, goal, seed, q):
    """make_cost_fn and make_is_solution_test_fn (src/goal.cpp:163-203) of one (goal, seed, q); `goal` holds
    x y z qw qx qy qz per tip frame, `params` the fields of pick_ik_amd.default_params()"""
    g = np.asarray(goal, dtype=np.float64).reshape(-1, 7)
    frames = fk(chain, q)
    lin = [linear_distance(t, gk[:3]) for (t, _), gk in zip(frames, g)]
    ang = [angular_distance(R, gk[3:]) for (_, R), gk in zip(frames, g)]
    c = sum((pose_cost(a, b, params.position_scale, params.rotation_scale) for a, b in zip(lin, ang)), M.mpf(0))
    terms = joint_goal_terms(chain, params, seed, q)
    c += sum((v * mpf(w) ** 2 for w, v in terms), M.mpf(0))
    sol = True  # thresholds are set only when the matching scale is > 0 (src/pick_ik_plugin.cpp:97-106)
    for a, b in zip(lin, ang):
        if params.position_scale > 0 and not a <= mpf(params.position_threshold):
            sol = False
        if params.rotation_scale > 0 and not b <= mpf(params.orientation_threshold):
            sol = False
    for w, v in terms:
        if not v * mpf(w) ** 2 < mpf(params.cost_threshold) ** 2:
            sol = False
    return Cost(c, sol, lin, ang, terms)


def reach(chain, q=None):
    """R of the error bounds: the sum of the norms of the origin and tip translations plus the prismatic extents
    (the largest |q| of a prismatic variable, from its limits or from `q`)"""
    r = 0.0
    for p in paths(chain):
        r += sum(float(np.linalg.norm(o[:3])) for o in p.origin_xyz_rpy) + float(np.linalg.norm(p.tip_xyz_rpy[:3]))
        for j, t in enumerate(p.joint_type):
            if int(t) in (robots.PRISMATIC, robots.PLANAR_X, robots.PLANAR_Y):
                v = int(p.variable[j])
                ext = max(abs(float(chain.qmin[v])), abs(float(chain.qmax[v])))
                if q is not None:
                    ext = max(ext, float(np.max(np.abs(np.asarray(q, dtype=np.float64).reshape(-1, chain.dof)[:, v]))))
                r += ext
    return r


def pose7(chain, q):
    """fk as doubles: x y z qw qx qy qz per tip (w >= 0), shape [7] or [n_tips][7] like Solver.fk"""
    out = []
    for t, R in fk(chain, q):
        out.append([float(x) for x in t] + [float(x) for x in matrix_to_quat(R)])
    out = np.array(out)
    return out if hasattr(chain, "tips") else out[0]


def pose_errors(chain, q, pose):
    """(position error [m], orientation error [rad]) per tip of a double pose (x y z qw qx qy qz, either sign of the
    quaternion) against the exact FK"""
    pose = np.asarray(pose, dtype=np.float64).reshape(-1, 7)
    out = []
    for (t, R), p in zip(fk(chain, q), pose):
        dp = float(M.sqrt(sum((a - mpf(b)) ** 2 for a, b in zip(t, p[:3]))))
        qe = matrix_to_quat(R)
        qp = [mpf(x) for x in p[3:]]
        # the angle between the two orientations, from the unnormalised double quaternion (its norm error is part
        # of the error: |q| - 1 enters every rotation the caller builds from it)
        n = M.sqrt(sum(x * x for x in qp))
        ang = quat_angle([x / n for x in qp], qe)
        out.append((dp, float(ang), float(abs(n - 1))))
    return out


@dataclasses.dataclass
class LineSearch:
    G_line: np.ndarray  # the gradient the line search ran with (doubles)
    line: tuple         # (Cost at fl(q - G_line), Cost at fl(q + G_line))
    p1: object          # their costs (mpf)
    p3: object
    p2: object          # (p1 + p3) / 2
    cost_diff: object   # (p3 - p1) / 2
    joint_diff: object  # p2 / cost_diff, 0 where that is not finite
    local: list         # clamp(q - G_line joint_diff), exact (mpf)


@dataclasses.dataclass
class Step:
    base: Cost          # cost at q
    probes: list        # per joint: (Cost at fl(q_j - h), Cost at fl(q_j + h))
    raw: list           # per joint: p3 - p1 of the probes (mpf)
    probe_width: list   # per joint: fl(q_j + h) - fl(q_j - h) (mpf, exact)
    f: object           # h / (h + sum |raw|) (mpf)
    G: list             # the normalised gradient raw * f (mpf)
    ls: LineSearch      # from the given G, or from G rounded to doubles
    local_cost: object  # cost at ls.local rounded to doubles (mpf)


def clamp(chain, j, v):
    """Variable::clamp_to_limits, src/robot.cpp:36-42 (an unbounded variable is left as it is)"""
    if int(chain.bounded[j]) == 0:
        return v
    lo, hi = mpf(chain.qmin[j]), mpf(chain.qmax[j])
    return lo if v < lo else hi if hi < v else v


def line_search(chain, params, goal, seed, q, G):
    """the second half of step(), src/ik_gradient.cpp:56-81, from the double gradient G: costs at the doubles
    fl(q -+ G), joint_diff = p2 / cost_diff (0 where not finite), the clamped update (exact)"""
    q, G = np.asarray(q, dtype=np.float64), np.asarray(G, dtype=np.float64)
    line = (cost(chain, params, goal, seed, q - G), cost(chain, params, goal, seed, q + G))
    p1, p3 = line[0].cost, line[1].cost
    p2 = (p1 + p3) / 2
    cd = (p3 - p1) / 2
    jd = p2 / cd if cd != 0 else M.mpf(0)
    local = [clamp(chain, j, mpf(q[j]) - mpf(G[j]) * jd) for j in range(len(q))]
    return LineSearch(G, line, p1, p3, p2, cd, jd, local)


def step(chain, params, goal, seed, q, G=None):
    """step() of src/ik_gradient.cpp:24-94 taken literally, every cost at PREC bits (`cost`): the probes at the
    doubles fl(q_j +- h), the gradient raw_j = p3 - p1 normalised by f = h / (h + sum |raw|), then `line_search`.
    `G` (doubles): run the line search from this gradient instead of the reference's own (rounded to doubles), so
    that it can be checked from a kernel's returned gradient separately from the gradient stage."""
    q = np.asarray(q, dtype=np.float64)
    h = float(params.gd_step_size)
    c = lambda x: cost(chain, params, goal, seed, x)  # noqa: E731
    base = c(q)
    probes, raw, width = [], [], []
    for j in range(len(q)):
        lo, hi = q.copy(), q.copy()
        lo[j] = q[j] - h  # (double arithmetic: the reference's working[i] = local[i] -+ step_size)
        hi[j] = q[j] + h
        probes.append((c(lo), c(hi)))
        raw.append(probes[-1][1].cost - probes[-1][0].cost)
        width.append(mpf(hi[j]) - mpf(lo[j]))
    hh = mpf(h)
    f = hh / (hh + sum(abs(g) for g in raw))
    Gm = [g * f for g in raw]
    ls = line_search(chain, params, goal, seed, q, np.array([float(g) for g in Gm]) if G is None else G)
    return Step(base, probes, raw, width, f, Gm, ls, c(np.array([float(x) for x in ls.local])).cost)
