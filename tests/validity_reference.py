"""The sphere validity test: the NORMATIVE code of include/pick_ik_amd.h (pikamd_validity_batch and the validity step
of the restart searches) in numpy, over any forward kinematics of the cut chains -- the CPU oracle's, or a handle's own
--, and the validated loops, built on tests/gate_reference.py by testing what its (gated) solve callables return.

A model is (spheres, pairs): spheres = [(after_variable, centre (3), radius), ...], pairs = [n_pairs][2] indices."""
import numpy as np

from pick_ik_amd import robots
from tests import gate_reference as G
from tests import search_global_reference as GR
from tests import search_reference as SR

VALIDITY_REFUSED = -1004


def centres(fk_of_cut_chain, model, q):
    """[n][n_spheres][3].  fk_of_cut_chain(after_variable, centre) -> fk(q [n][after_variable + 1]) -> [n][7]: the
    forward kinematics of robots.cut_chain(chain, after_variable, centre).  A base-frame sphere is copied."""
    spheres, _ = model
    q = np.asarray(q, dtype=np.float64)
    out = np.empty((len(q), len(spheres), 3))
    for k, (after, c, _r) in enumerate(spheres):
        if after < 0:
            out[:, k] = np.asarray(c, dtype=np.float64)
        else:
            out[:, k] = np.asarray(fk_of_cut_chain(after, c)(np.ascontiguousarray(q[:, :after + 1])))[:, :3]
    return out


def pair_clearances(model, cen):
    """clear_m [n][n_pairs]: every operation rounded on its own (numpy float64 arithmetic is), IEEE square root"""
    spheres, pairs = model
    pairs = np.asarray(pairs, dtype=np.int64).reshape(-1, 2)
    r = np.array([s[2] for s in spheres], dtype=np.float64)
    i, j = pairs[:, 0], pairs[:, 1]
    with np.errstate(invalid="ignore"):
        d = cen[:, i] - cen[:, j]
        dx, dy, dz = d[..., 0], d[..., 1], d[..., 2]
        d2 = (dx * dx + dy * dy) + dz * dz
        return np.sqrt(d2) - (r[i] + r[j])


def clearance(model, cen):
    """[n]: +infinity, then every clear_m that is smaller in ascending m (a NaN never replaces)"""
    cl = pair_clearances(model, cen)
    out = np.full(len(cen), np.inf)
    with np.errstate(invalid="ignore"):
        for m in range(cl.shape[1]):
            out = np.where(cl[:, m] < out, cl[:, m], out)
    return out


def valid(model, cen):
    """[n] bool: no clear_m < 0.0 (a NaN does not trip the test; touching spheres are valid)"""
    with np.errstate(invalid="ignore"):
        return ~(pair_clearances(model, cen) < 0.0).any(axis=1)


def oracle_fk_of(O, chain):
    """fk_of_cut_chain over the CPU oracle, in the math mode that is set when it is CALLED"""
    cache = {}

    def fk_of(after, c):
        key = (after, tuple(c))
        if key not in cache:
            cache[key] = O.Oracle(robots.cut_chain(chain, after, c))
        return cache[key].fk
    return fk_of


def handle_fk_of(make_solver, chain):
    """fk_of_cut_chain over handles made by make_solver(cut chain) (closed by close_all(fk_of))"""
    cache = {}

    def fk_of(after, c):
        key = (after, tuple(c))
        if key not in cache:
            cache[key] = make_solver(robots.cut_chain(chain, after, c))
        return cache[key].fk
    fk_of.cache = cache
    return fk_of


def close_all(fk_of):
    for s in fk_of.cache.values():
        s.close()
    fk_of.cache.clear()


def valid_of(fk_of_cut_chain, model):
    """q [n][dof] -> valid [n], or None without a model"""
    if model is None:
        return None
    return lambda q: valid(model, centres(fk_of_cut_chain, model, q))


def validated(solve, valid_fn):
    """The step the model adds behind a (gated) solve: solve(goals, seed, ...) -> (solution, status, cost, stats) with
    every answer of status > 0 that valid_fn(solution) refuses turned into (seed, VALIDITY_REFUSED); cost and stats stay.
    valid_fn None (no model): `solve` itself."""
    if valid_fn is None:
        return solve

    def validated_solve(goals, seed, *rest):
        sol, st, c, stats = solve(goals, seed, *rest)
        sol, st = np.array(sol), np.array(st)
        idx = np.nonzero(st > 0)[0]
        if len(idx):
            bad = idx[~np.asarray(valid_fn(sol[idx]), dtype=bool)]
            st[bad] = VALIDITY_REFUSED
            sol[bad] = np.asarray(seed)[bad]
        return sol, st, c, stats
    return validated_solve


def oracle_search(O, chain, goals, seed, max_attempts, kw, gate, model, **search_kw):
    """the gated and validated local-mode loop over the CPU oracle, in the math mode that is set"""
    o = O.Oracle(chain)
    p = O.default_params(mode=1, **kw)
    solve = G.gated(lambda g, sd, ig: o.solve_batch(p, g, sd, num_threads=O.max_threads(), initial_guess=ig),
                    G.oracle_cost(o), p, gate)
    return SR.reference_search(validated(solve, valid_of(oracle_fk_of(O, chain), model)), chain, goals, seed, max_attempts,
                               **search_kw)


def oracle_search_global(O, chain, goals, seed, max_attempts, kw, gate, model, **search_kw):
    """... and the global-mode one"""
    o = O.Oracle(chain)
    p = O.default_params(mode=0, **kw)
    solve = G.gated(GR.oracle_solve_one(O, chain, p), G.oracle_cost(o), p, gate)
    return GR.reference_search(validated(solve, valid_of(oracle_fk_of(O, chain), model)), chain, goals, seed, max_attempts,
                               **search_kw)


def handle_search(s, p, gate, chain, goals, seed, max_attempts, **search_kw):
    """the local-mode loop over a handle's own solve_batch, gate and validity (the model set on the handle)"""
    solve = G._handle_gated(lambda g, sd, ig: s.solve_batch(p, g, sd, initial_guess=ig), s, p, gate)
    return SR.reference_search(validated(solve, lambda q: s.validity(q)[0]), chain, goals, seed, max_attempts, **search_kw)


def handle_search_global(s, p, gate, chain, goals, seed, max_attempts, **search_kw):
    """the loop over a handle's own solve_batches, gate and validity (the model set on the handle): the definition,
    for every flavour"""
    solve = G._handle_gated(GR.handle_solve_one(s, p), s, p, gate)
    return GR.reference_search(validated(solve, lambda q: s.validity(q)[0]), chain, goals, seed, max_attempts, **search_kw)


def fixture_counts(all_status_plain, all_status, status, attempts):
    """Of a call's attempt rows without the model (all_status_plain [B][K]) and with it (all_status, status, attempts):
    (solved and refused at attempt 0, solved and valid at attempt 0, rescued at an attempt >= 1 after a validity refusal,
    ending VALIDITY_REFUSED)"""
    refused0 = (all_status_plain[:, 0] > 0) & (all_status[:, 0] == VALIDITY_REFUSED)
    valid0 = all_status[:, 0] > 0
    had_refusal = np.array([(all_status[b, :max(int(attempts[b]) - 1, 0)] == VALIDITY_REFUSED).any()
                            for b in range(len(status))])
    rescued = (status > 0) & (attempts > 1) & had_refusal
    return int(refused0.sum()), int(valid0.sum()), int(rescued.sum()), int((status == VALIDITY_REFUSED).sum())
