"""The validity model inside the path entry points (pikamd_set_path_validity): the NORMATIVE loop of
include/pick_ik_amd.h -- pikamd_solve_paths' loop with the one extra step `refused` -- over any solve_batch-shaped
callable plus a valid_fn (validity_reference.valid_of, or a handle's own validity), and pikamd_cartesian_paths /
pikamd_cartesian_waypoints composed over it.  path_reference.reference_paths, cartesian_reference.reference_cartesian
and polyline_reference.reference_polyline are used as they are: the step is put behind the solve callable they take.

Two forms.  The DEFINITION: the walk stops at the refused answer (refusing + the three loops).  The POST-PASS, which is
how the device does it: the plain result, then the cut (cut_paths, cut_cartesian).  tests/test_pathvalid_cpu.py holds
them to one another on the fixtures.

The fixture rule "placed obstacles": obstacles put, by construction, on the hand sphere of chosen rows of paths that
are complete and collision-free without them."""
import numpy as np

from pick_ik_amd import robots
from tests import cartesian_reference as CR
from tests import path_reference as PR
from tests import polyline_reference as LR

VALIDITY_REFUSED = -1004
HAND_SPHERE = 7
OBSTACLE_RADIUS = 0.03
N_OBSTACLES = 12
ZERO_STATS = np.zeros((), dtype=PR.STATS_DTYPE)


# ---- the definition ---------------------------------------------------------------------------------
def refusing(solve, valid_fn, max_joint_step=None):
    """The extra step of the loop, behind the solve of one waypoint: an answer of status > 0 that the joint-step test
    lets pass (a jumped answer is not tested: the loop around makes it PATH_JUMP) and valid_fn refuses comes back as
    (seed, VALIDITY_REFUSED) -- what the loop stores for a failed waypoint --, its cost and counters as they are.
    valid_fn None (the switch off, or no model): `solve` itself."""
    if valid_fn is None:
        return solve
    lim = None if max_joint_step is None else np.asarray(max_joint_step, dtype=np.float64)

    def solve_and_test(goals, seed):
        sol, st, c, stats = solve(goals, seed)
        sol, st, seed = np.array(sol), np.array(st), np.asarray(seed, dtype=np.float64)
        test = st > 0
        if lim is not None:
            with np.errstate(invalid="ignore"):
                test &= ~np.any((lim > 0.0) & (np.abs(sol - seed) > lim), axis=1)
        idx = np.nonzero(test)[0]
        if len(idx):
            bad = idx[~np.asarray(valid_fn(sol[idx]), dtype=bool)]
            st[bad] = VALIDITY_REFUSED
            sol[bad] = seed[bad]
        return sol, st, c, stats
    return solve_and_test


def reference_paths(solve, goals, start, max_joint_step=None, valid_fn=None):
    """pikamd_solve_paths with the step: (solution, status, cost, stats, reached)"""
    return PR.reference_paths(refusing(solve, valid_fn, max_joint_step), goals, start, max_joint_step)


def reference_cartesian(solve, goals, steps, start, jump_factor=0.0, max_joint_step=None, valid_fn=None):
    """pikamd_cartesian_paths with the step: cartesian_reference.reference_cartesian's return"""
    return CR.reference_cartesian(refusing(solve, valid_fn, max_joint_step), goals, steps, start, jump_factor,
                                  max_joint_step)


def reference_polyline(solve, fk, interpolate, cartesian, start, targets, W, n_targets=None, max_joint_step=None,
                       valid_fn=None):
    """pikamd_cartesian_waypoints with the step: polyline_reference.reference_polyline's return"""
    return LR.reference_polyline(refusing(solve, valid_fn, max_joint_step), fk, interpolate, cartesian, start, targets,
                                 W, n_targets, max_joint_step)


# ---- the post-pass ------------------------------------------------------------------------------------
def first_refused(solution, reached, valid_fn):
    """f [P]: the first of rows 0 .. reached[p] - 1 that valid_fn refuses, or -1"""
    P, W = solution.shape[:2]
    f = np.full(P, -1, dtype=np.int64)
    rows = [(p, k) for p in range(P) for k in range(int(reached[p]))]
    if rows:
        pp, kk = np.array(rows).T
        ok = np.asarray(valid_fn(np.ascontiguousarray(solution[pp, kk])), dtype=bool)
        for p, k in zip(pp[~ok][::-1], kk[~ok][::-1]):
            f[p] = k
    return f


def _cut_row(solution, status, cost, stats, start, p, f):
    held = start[p] if f == 0 else solution[p, f - 1].copy()
    solution[p, f:] = held
    status[p, f] = VALIDITY_REFUSED
    status[p, f + 1:] = PR.NOT_ATTEMPTED
    cost[p, f + 1:] = 0.0
    stats[p, f + 1:] = ZERO_STATS


def cut_paths(plain, start, valid_fn):
    """the plain result of pikamd_solve_paths (five arrays), cut: row f the held state and VALIDITY_REFUSED with its
    cost and counters, the rows behind it blank, reached = f"""
    solution, status, cost, stats, reached = (np.array(x) for x in plain)
    start = np.asarray(start, dtype=np.float64)
    f = first_refused(solution, reached, valid_fn)
    for p in np.nonzero(f >= 0)[0]:
        _cut_row(solution, status, cost, stats, start, p, int(f[p]))
        reached[p] = f[p]
    return solution, status, cost, stats, reached


def cut_cartesian(plain0, start, W, jump_factor, valid_fn, f=None):
    """the plain result of pikamd_cartesian_paths WITH jump_factor 0 (seven arrays), cut, and then the tail: fraction
    = r / n and the relative test over the cut path.  A path with steps > W is left alone.  f [P]: the first refused
    rows where the caller has them already (-1: none), else valid_fn finds them."""
    solution, status, cost, stats, reached, steps, fraction = (np.array(x) for x in plain0)
    start = np.asarray(start, dtype=np.float64)
    if f is None:
        f = first_refused(solution, np.where(steps <= W, reached, 0), valid_fn)
    for p in range(len(steps)):
        n = int(steps[p])
        if n > W:
            continue
        if f[p] >= 0:
            _cut_row(solution, status, cost, stats, start, p, int(f[p]))
            reached[p] = f[p]
        r = int(reached[p])
        fraction[p] = np.float64(r) / np.float64(n)
        if jump_factor > 0.0 and r >= 1:
            traj = np.concatenate([start[p][None], solution[p, :r]])
            i = CR.relative_jump(traj, jump_factor)
            if i is not None:
                fraction[p] = fraction[p] * (np.float64(i + 1) / np.float64(r + 1))
                solution[p, i:] = traj[i]
                status[p, i] = CR.PATH_RELATIVE_JUMP
                status[p, i + 1:] = CR.NOT_ATTEMPTED
                cost[p, i + 1:] = 0.0
                stats[p, i + 1:] = ZERO_STATS
                reached[p] = i
    return solution, status, cost, stats, reached, steps, fraction


# ---- the fixtures -------------------------------------------------------------------------------------
def place_obstacles(centres_fn, valid0_fn, solution, complete, start, W, n=N_OBSTACLES, first=3, stride=5):
    """The rule: of the paths whose plain walk is complete (complete [P]), whose start the robot-only model holds valid
    and none of whose rows it refuses, the first n; for the i-th an obstacle of OBSTACLE_RADIUS at the centre of the
    hand sphere at row (first + stride * i) mod W.  centres_fn(q) -> [n][n_spheres][3] and valid0_fn(q) -> [n] are the
    robot-only model's (robots.panda_spheres(obstacles=())).  Returns (obstacles, chosen paths, their rows)."""
    P = solution.shape[0]
    ok = np.asarray(valid0_fn(np.asarray(start)), dtype=bool)
    rows_ok = np.asarray(valid0_fn(solution.reshape(P * W, -1)), dtype=bool).reshape(P, W)
    chosen = [p for p in range(P) if complete[p] and ok[p] and rows_ok[p].all()][:n]
    rows = [(first + stride * i) % W for i in range(len(chosen))]
    obstacles = []
    for p, k in zip(chosen, rows):
        c = centres_fn(solution[p, k][None])[0, HAND_SPHERE]
        obstacles.append(((float(c[0]), float(c[1]), float(c[2])), OBSTACLE_RADIUS))
    return tuple(obstacles), chosen, rows


def cut_classes(plain_status, plain_reached, status, reached, n_rows):
    """Of a fixture walked without (plain_*) and with the model: (complete paths the model leaves alone, paths cut at
    row 0, paths cut inside, the distinct rows of those, paths the solver had already stopped that are cut in front of
    that stop).  n_rows [P] or int: the rows a complete path has."""
    P = status.shape[0]
    n_rows = np.broadcast_to(np.asarray(n_rows), (P,))
    cut = (status == VALIDITY_REFUSED).any(axis=1)
    at = np.array([int(np.argmax(status[p] == VALIDITY_REFUSED)) if cut[p] else -1 for p in range(P)])
    complete = plain_reached == n_rows
    alone = complete & ~cut & (reached == n_rows)
    inside = cut & (at > 0)
    stopped = cut & ~complete
    return (int(alone.sum()), int((cut & (at == 0)).sum()), int(inside.sum()), len(set(at[inside].tolist())),
            int(stopped.sum()))


#: what the fixture "placed obstacles" must reach (the issue's minima): complete and left alone, cut at row 0, cut
#: inside, distinct inside rows, cut on a solver-stopped path
MINIMA_PATHS = (8, 4, 8, 6, 1)


def panda_model(obstacles):
    """(spheres, pairs) of the Panda with these obstacles, as Solver.set_validity_model and validity_reference take it"""
    return robots.panda_spheres(obstacles=obstacles)


# ---- the three fixtures over the CPU oracle (computed once per math mode, left unchanged) ---------------
P_PATHS, W_PATHS = 64, 32
W_OFFSETS = 12
_memo = {}


def _oracle_tools(O, chain):
    from tests import validity_reference as V
    o = O.Oracle(chain)
    po = O.default_params(mode=1)
    solve = lambda g, sd: o.solve_batch(po, g, sd, num_threads=O.max_threads())
    fk_of = V.oracle_fk_of(O, chain)
    robot = panda_model(())
    return o, solve, fk_of, (lambda q: V.centres(fk_of, robot, q)), V.valid_of(fk_of, robot), V


def _frozen(*arrays):
    for a in arrays:
        if isinstance(a, np.ndarray):
            a.setflags(write=False)


def placed_paths(O, mode):
    """The fixture "placed obstacles" over the oracle in one math mode: dict(chain, goals, start, model, plain, want,
    chosen, rows) -- plain: the walk without a model, want: the loop with the step."""
    key = ("paths", mode)
    if key not in _memo:
        chain = robots.panda()
        with O.math_mode(mode):
            o, solve, fk_of, centres_fn, valid0, V = _oracle_tools(O, chain)
            goals, start = PR.straight_lines(chain, o.fk, P=P_PATHS, W=W_PATHS)
            plain = PR.reference_paths(solve, goals, start)
            obstacles, chosen, rows = place_obstacles(centres_fn, valid0, plain[0], plain[4] == W_PATHS, start, W_PATHS)
            model = panda_model(obstacles)
            want = reference_paths(solve, goals, start, None, V.valid_of(fk_of, model))
        _frozen(goals, start, *plain, *want)
        _memo[key] = dict(chain=chain, goals=goals, start=start, model=model, plain=plain, want=want, chosen=chosen,
                          rows=rows)
    return _memo[key]


#: the placement on the Cartesian fixtures: fewer obstacles than on "placed obstacles" (their starts lie close together,
#: and every obstacle cuts its neighbours at row 0 as well), every second one on the LAST row of its path, so that a
#: relative stop in front of it can survive the cut
N_CARTESIAN, FIRST_CARTESIAN, STRIDE_CARTESIAN = 4, 3, 5
#: ... and, on "panda offsets", this many more on complete paths that have a relative stop (the fixture's jump_factor,
#: no model) in front of their last row: on the last row f for which the first row the obstacle refuses -- the hand is
#: within the two radii of where it is at row f -- lies behind the stop, and the relative test over the rows in front
#: of that one still stops where it did
N_SURVIVORS = 2
HAND_RADIUS = 0.07


def _surviving_row(start_p, rows_p, hand, n, stop, jump_factor):
    for f in range(n - 1, stop, -1):
        near = np.linalg.norm(hand[:n] - hand[f], axis=1) < HAND_RADIUS + OBSTACLE_RADIUS
        cut = int(np.argmax(near))
        if cut > stop and CR.relative_jump(np.concatenate([start_p[None], rows_p[:cut]]), jump_factor) == stop:
            return f
    return None


def _placed_rows(counts, chosen, first=FIRST_CARTESIAN, stride=STRIDE_CARTESIAN):
    """the i-th chosen path's row: (first + stride i) mod its rows for even i, its last row for odd i"""
    return [((first + stride * i) % int(counts[p])) if i % 2 == 0 else int(counts[p]) - 1 for i, p in enumerate(chosen)]


def _obstacles_at(centres_fn, solution, chosen, rows):
    out = []
    for p, k in zip(chosen, rows):
        c = centres_fn(solution[p, k][None])[0, HAND_SPHERE]
        out.append(((float(c[0]), float(c[1]), float(c[2])), OBSTACLE_RADIUS))
    return tuple(out)


def placed_offsets(O, pk, mode, limit=None, n=N_CARTESIAN, survivors=N_SURVIVORS):
    """The fixture "panda offsets" (W 12, cartesian_reference.OFFSETS) with obstacles placed on the first n paths that
    are complete without the relative test, collision-free and valid at the start (_placed_rows says where).
    dict(chain, start, target, goals, steps, model, plain0 (jump_factor 0, no model), plain (the fixture's jump_factor,
    no model), want, held_plain, held)."""
    key = ("offsets", mode, limit, n, survivors)
    if key not in _memo:
        chain = robots.panda()
        W, jf = W_OFFSETS, CR.OFFSETS["jump_factor"]
        step = None if limit is None else np.full(chain.dof, limit)
        with O.math_mode(mode):
            o, solve, fk_of, centres_fn, valid0, V = _oracle_tools(O, chain)
            start, target = CR.offsets(chain)
            goals, steps = pk.interpolate_poses(pk.Cartesian(**CR.OFFSETS), o.fk(start), target, W, strict=mode == "portable")
            pkey = ("offsets plain", mode, limit)
            if pkey not in _memo:
                _memo[pkey] = (CR.reference_cartesian(solve, goals, steps, start, 0.0, step)[0],
                               CR.reference_cartesian(solve, goals, steps, start, jf, step))
            plain0, (plain, held_plain) = _memo[pkey]
            P = len(start)
            ok = np.asarray(valid0(start), dtype=bool)
            rows_ok = np.asarray(valid0(plain0[0].reshape(P * W, -1)), dtype=bool).reshape(P, W)
            chosen = [p for p in range(P) if steps[p] <= W and plain0[4][p] == steps[p] and ok[p] and rows_ok[p].all()][:n]
            rows = _placed_rows(steps, chosen)
            rel = plain[1] == CR.PATH_RELATIVE_JUMP
            more = []
            for p in range(P):
                if len(more) < survivors and p not in chosen and steps[p] <= W and plain0[4][p] == steps[p] and ok[p] \
                        and rows_ok[p].all() and rel[p].any():
                    f = _surviving_row(start[p], plain0[0][p], centres_fn(plain0[0][p])[:, HAND_SPHERE], int(steps[p]),
                                       int(np.argmax(rel[p])), jf)
                    if f is not None:
                        more.append((p, f))
            chosen, rows = chosen + [p for p, _ in more], rows + [f for _, f in more]
            model = panda_model(_obstacles_at(centres_fn, plain0[0], chosen, rows))
            want, held = reference_cartesian(solve, goals, steps, start, jf, step, V.valid_of(fk_of, model))
        _frozen(start, target, goals, steps, *plain0, *plain, *want)
        _memo[key] = dict(chain=chain, start=start, target=target, goals=goals, steps=steps, model=model, plain0=plain0,
                          plain=plain, want=want, held_plain=held_plain, held=held, chosen=chosen, rows=rows)
    return _memo[key]


def placed_polylines(O, pk, mode, limit=None, n=N_CARTESIAN):
    """The fixture "panda polylines" (S 3, W 16, polyline_reference.POLYLINES) with obstacles placed by the same rule on
    the paths every segment of which holds without the relative test, over the stitched rows.  dict(chain, start,
    targets, n_targets, model, plain, info_plain, want, info)."""
    key = ("polylines", mode, limit, n)
    if key not in _memo:
        chain = robots.panda()
        S, W = LR.S_POLYLINES, LR.W_POLYLINES
        step = None if limit is None else np.full(chain.dof, limit)
        kw0 = dict(LR.POLYLINES, jump_factor=0.0)
        with O.math_mode(mode):
            o, solve, fk_of, centres_fn, valid0, V = _oracle_tools(O, chain)
            start, targets, n_targets = LR.polylines(chain)
            interp = lambda c, a, t, w: pk.interpolate_poses(c, a, t, w, strict=mode == "portable")
            pkey = ("polylines plain", mode, limit)
            if pkey not in _memo:
                _memo[pkey] = (LR.reference_polyline(solve, o.fk, interp, pk.Cartesian(**kw0), start, targets, W, n_targets, step),
                               LR.reference_polyline(solve, o.fk, interp, pk.Cartesian(**LR.POLYLINES), start, targets, W,
                                                     n_targets, step))
            (plain0, info0), (plain, info_plain) = _memo[pkey]
            P = len(start)
            ok = np.asarray(valid0(start), dtype=bool)
            rows_ok = np.asarray(valid0(plain0[0].reshape(P * W, -1)), dtype=bool).reshape(P, W)
            chosen = [p for p in range(P) if info0["kind"][p] == LR.COMPLETE and info0["held"][p] >= 1 and ok[p]
                      and rows_ok[p].all()][:n]
            rows = _placed_rows(info0["held"], chosen)
            model = panda_model(_obstacles_at(centres_fn, plain0[0], chosen, rows))
            want, info = reference_polyline(solve, o.fk, interp, pk.Cartesian(**LR.POLYLINES), start, targets, W, n_targets,
                                            step, V.valid_of(fk_of, model))
        _frozen(start, targets, n_targets, *plain, *want)
        _memo[key] = dict(chain=chain, start=start, targets=targets, n_targets=n_targets, model=model, plain=plain,
                          info_plain=info_plain, info0=info0, want=want, info=info, chosen=chosen, rows=rows)
    return _memo[key]


def cartesian_classes(plain_status, held_plain, rows_of, status, held):
    """Of a Cartesian fixture (the fixture's jump_factor) without and with the model.  held_plain, held [P]: the rows
    held before the relative test; rows_of [P]: the rows a complete path has (-1: the plain walk was not complete).
    dict(alone: complete paths the model leaves alone; inside: paths cut inside; at0: paths cut at row 0; moved: cut
    paths whose relative stop moves, vanishes or appears; survives: cut paths that keep their relative stop, in front
    of the cut)."""
    at = lambda m: np.where(m.any(axis=1), np.argmax(m, axis=1), -1)
    f = at(status == VALIDITY_REFUSED)
    r, r0 = at(status == CR.PATH_RELATIVE_JUMP), at(plain_status == CR.PATH_RELATIVE_JUMP)
    cut = held < held_plain
    assert (cut | (held == held_plain)).all()
    alone = (held_plain == rows_of) & ~cut
    return dict(alone=int(alone.sum()), inside=int((cut & (held > 0)).sum()), at0=int((cut & (held == 0)).sum()),
                moved=int((cut & (r != r0)).sum()), survives=int((cut & (r0 >= 0) & (r == r0)).sum()),
                shown=int((f >= 0).sum()))


def cut_behind_the_first_segment(held_plain, held, segment_steps, seg):
    """paths of a waypoint-list fixture that the model cuts in a segment behind the first"""
    return int(((held < held_plain) & (held >= segment_steps[:, 0]) & (seg >= 1)).sum())


MINIMA_CARTESIAN = dict(alone=4, inside=4, at0=1, moved=1, survives=1)
