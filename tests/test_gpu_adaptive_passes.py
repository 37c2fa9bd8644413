"""The adaptive compaction passes (launch_solve's range table, pik_launch.hpp) and the routed launcher in front of them
(pik_route.hpp) on every chain length, elite group size and kernel family -- small calls that are nevertheless cut into
passes: the option "passes" is set (which keeps a small call from being served by one launch) and "lanes_per_elite" is
left alone (which keeps the call adaptive and eligible for the routers).

Every solve asserts what served it: the namespace of pikamd_kernel_name, and the routers' record
(pikamd_debug_regime) -- one entry per pass, the first one the call's size, every entry the decision of
tests/route_model.py (a restatement of DESIGN.md section 4 that does not call the library), and no record at all under
device_regime = 0.  Results are compared at tolerance zero on solution, status, cost and stats: exact handles with the
oracle in math mode "fma", fast handles with the same handle at one lane per elite without passes (ONE launch, no
router: the shape tests/test_gpu_product_arithmetic.py ties to the host execution), their SUCCESS rows also with the
oracle's own solution test.

About a fifth of the targets of a call are out of reach, so that every pass has survivors; the other targets start
from seeds at graded distances from a solution, so that the survivor counts fall from mark to mark.  The seeds of the
generated cases are chosen (on the CPU, with the oracle) so that under load the survivor counts cross the border
between the two one-lane variants."""
import os
import subprocess
import sys

import numpy as np
import pytest

import pick_ik_amd as pk
from pick_ik_amd import robots
from tests import route_model as M
from tests.test_gpu_device_regime import simds  # noqa: F401  (the fixture: SIMDs from the topology files)
from tests.test_gpu_fuzz import common_case, random_chain

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYNC_SLOT = pk.solver.MAX_SLOTS + pk.solver.MAX_HOST_JOBS - 1  # the slot of the synchronous host-pointer calls
LOAD_SLOT = 5  # a device slot no call of this file uses: carries the artificial load
NAMES = ("solution", "status", "cost", "stats")
FAR = 50.0  # metres added to a target's position: out of reach of every chain here (16 links of at most 0.61 m)


@pytest.fixture(scope="module")
def O(oracle_mod):
    import __graft_entry__ as g
    g.build()
    return oracle_mod


def assert_same(a, b, what):
    for x, y, w in zip(a, b, NAMES):
        np.testing.assert_array_equal(x, y, err_msg=f"{what}: {w}")


def effective_marks(marks, generations):
    """the marks a call keeps: ascending, below the generation budget, at most fifteen"""
    out = []
    for m in marks:
        if 0 < m < generations and (not out or m > out[-1]) and len(out) < 15:
            out.append(m)
    return out


def problems(o, ch, rng, B, unreachable=None, sigma=(1e-3, 1.0)):
    """(goal, seed): targets of random configurations; the first `unreachable` (default: a fifth) pushed out of reach;
    the seeds of the others at graded distances from the configuration behind the target"""
    lo = np.where(np.asarray(ch.bounded) == 1, ch.qmin, -3.0)
    hi = np.where(np.asarray(ch.bounded) == 1, ch.qmax, 3.0)
    q = rng.uniform(lo, hi, size=(B, ch.dof))
    goal = o.fk(q)
    k = B // 5 if unreachable is None else unreachable
    goal[:k, :3] += FAR
    s = np.exp(rng.uniform(np.log(sigma[0]), np.log(sigma[1]), size=(B, 1)))
    seed = np.clip(q + s * rng.normal(size=q.shape), lo, hi)
    return goal, seed


class Call:
    """one call's inputs, its marks and the model of the variants it is offered"""

    def __init__(self, ch, kw, goal, seed, rs, off, marks, model):
        self.ch, self.kw, self.goal, self.seed, self.rs, self.off = ch, kw, goal, seed, rs, off
        self.marks, self.model = marks, model
        self.B = len(goal)
        self.n_passes = len(effective_marks(marks, kw["memetic_max_generations"])) + 1
        assert 24 <= self.B <= 160 and self.B % 64 != 0
        # (population 12 .. 72; the elite group sizes 1 .. 3 of case b come with elites + 8 = 9 .. 11)
        assert 9 <= kw["memetic_population_size"] <= 72 and kw["memetic_max_generations"] <= 16
        assert kw.get("memetic_gd_max_iters", 25) <= 25

    def params(self, mod=pk):
        return mod.default_params(**self.kw)

    def passes(self):
        return ",".join(str(m) for m in self.marks)


def routed(s, c, load, slot=SYNC_SLOT):
    """the call through the routers under an artificial load on LOAD_SLOT: (results, record)"""
    s.set_option("device_regime", "1")
    s.set_option("lanes_per_elite", None)
    s.set_option("passes", c.passes())
    s.debug_regime(LOAD_SLOT, publish_load=load)
    try:
        got = s.solve_batch(c.params(), c.goal, c.seed, rng_seed=c.rs, problem_offset=c.off)
    finally:
        rec = s.debug_regime(slot)
        s.debug_regime(LOAD_SLOT, publish_load=0)
    return got, rec


def check_routed(s, c, load, ref, what, threshold=None):
    got, rec = routed(s, c, load)
    print(f"{what} load {load}: (survivors, others' load, variant) per pass = {rec}")
    assert rec is not None and len(rec) == c.n_passes, (what, rec)
    ids = c.model.check_record(rec, c.B, load, threshold)
    assert_same(got, ref, f"{what} load {load}")
    return rec, ids


def host_rule(s, c, ref, what):
    """device_regime = 0 and the same marks: launch_solve's adaptive table, every variant of it enqueued"""
    s.set_option("device_regime", "0")
    s.set_option("lanes_per_elite", None)
    s.set_option("passes", c.passes())
    try:
        got = s.solve_batch(c.params(), c.goal, c.seed, rng_seed=c.rs, problem_offset=c.off)
        assert s.debug_regime(SYNC_SLOT) is None, what
    finally:
        s.set_option("device_regime", "1")
    assert_same(got, ref, f"{what} device_regime 0")


def reference(s, o, O, c, namespace, what):
    """what the call has to return: an exact handle's from the oracle, a fast handle's from its own one-lane launch"""
    assert s.kernel_name(c.params()).startswith(namespace + "::"), (what, s.kernel_name(c.params()))
    if namespace == "pik_exact":
        with O.math_mode("fma"):
            return o.solve_batch(c.params(O), c.goal, c.seed, rng_seed=c.rs, problem_offset=c.off,
                                 num_threads=O.max_threads())
    s.set_option("lanes_per_elite", 1)
    s.set_option("passes", "none")
    ref = s.solve_batch(c.params(), c.goal, c.seed, rng_seed=c.rs, problem_offset=c.off)
    assert s.debug_regime(SYNC_SLOT) is None, what
    s.set_option("lanes_per_elite", None)
    sol, st, cost, _ = ref
    op = c.params(O)
    for b in np.flatnonzero(st == pk.SUCCESS)[:40]:
        cc, is_sol = o.cost(op, c.goal[b], c.seed[b], sol[b])
        assert is_sol[0] == 1, f"{what} problem {b}: SUCCESS but the oracle rejects (cost {cc[0]})"
        assert abs(cc[0] - cost[b]) <= 1e-9 * max(1.0, abs(cc[0]))
    return ref


# ---- a. chain lengths 1..16 across the four product families -------------------------------------------------------

FAMILIES = ("pik_common", "pik_common_goals", "pik", "pik_exact")
A_MARKS = (1, 2, 4, 7, 10, 13)
#: (family, D) -> the draw of the problems and parameters that is taken: the first one for which, by the oracle on the
#: CPU (math mode "fma"), at least 38 problems are still running at some mark, at most 27 at another, and 40 or more
#: succeed -- under load the passes of such a call lie on both sides of the border between the two one-lane variants
#: (31 | 32 problems for four elites and two_per_simd = 2); a case without an entry takes draw 0
A_PROBLEM_DRAW = {
    ("pik_common", 1): 1, ("pik_common", 2): 1, ("pik_common", 4): 1, ("pik_common", 5): 22, ("pik_common", 6): 178,
    ("pik_common", 7): 67, ("pik_common", 8): 18, ("pik_common", 9): 14, ("pik_common", 10): 1,
    ("pik_common", 11): 5, ("pik_common", 12): 26, ("pik_common", 13): 1, ("pik_common", 14): 2,
    ("pik_common", 15): 16,
    ("pik_common_goals", 1): 11, ("pik_common_goals", 3): 16, ("pik_common_goals", 4): 9,
    ("pik_common_goals", 5): 77, ("pik_common_goals", 6): 231, ("pik_common_goals", 7): 1,
    ("pik_common_goals", 8): 20, ("pik_common_goals", 9): 59, ("pik_common_goals", 10): 31,
    ("pik_common_goals", 11): 1, ("pik_common_goals", 12): 41, ("pik_common_goals", 13): 67,
    ("pik_common_goals", 14): 1, ("pik_common_goals", 15): 6, ("pik_common_goals", 16): 4,
    ("pik", 3): 3, ("pik", 5): 5, ("pik", 6): 16, ("pik", 7): 64, ("pik", 8): 46, ("pik", 9): 49, ("pik", 10): 20,
    ("pik", 11): 36, ("pik", 14): 3, ("pik", 15): 2, ("pik", 16): 3,
    ("pik_exact", 1): 1, ("pik_exact", 2): 6, ("pik_exact", 3): 2, ("pik_exact", 5): 1, ("pik_exact", 6): 74,
    ("pik_exact", 7): 4, ("pik_exact", 8): 3, ("pik_exact", 10): 11, ("pik_exact", 12): 23, ("pik_exact", 15): 2,
}
#: (family, D) -> the draw of the chain where the first one is not taken: no draw of 400 with common_case's first
#: six-variable chain and joint goals lets 40 problems converge within 16 generations
A_CHAIN_DRAW = {("pik_common_goals", 6): 1}


def family_chain(family, D):
    """the chain of a case: common-configuration chains as tests/test_gpu_fuzz.py common_case draws them, the others
    by random_chain (prismatic, continuous, planar and unbounded variables; the general family's chain of 15 variables
    has a pair of nearly parallel axes: a general Denavit-Hartenberg step, no cooperative descent)"""
    t = A_CHAIN_DRAW.get((family, D), 0)
    if family.startswith("pik_common"):
        # (common_case(i): D = 1 + i % 16; a chain with an ill-conditioned pair of axes would be served by pik::)
        return common_case(D - 1 + 16 * t)[0]
    base = 0xADA if family == "pik" else 0xE8AC
    return random_chain(np.random.default_rng([base, D, t]), D)


def family_call(O, family, D, simds, draw=None):
    ch = family_chain(family, D)
    t = A_PROBLEM_DRAW.get((family, D), 0) if draw is None else draw
    rng = np.random.default_rng([FAMILIES.index(family), D, t])
    kw = dict(memetic_population_size=int(rng.integers(12, 73)), memetic_max_generations=16,
              memetic_gd_max_iters=int(rng.choice([0, 1, 5, 12, 25])),
              gd_step_size=float(rng.choice([1e-4, 1e-3, 1e-5])),
              position_threshold=float(rng.choice([1e-3, 1e-5, 1e-7])),
              orientation_threshold=float(rng.choice([1e-3, 1e-5, 1e-7])),
              # (three elites on the general kernels: four of them on a bounded revolute chain are pik_common's)
              memetic_elite_size=3 if family == "pik" else 4)
    if family == "pik_common_goals":
        kw.update(center_joints_weight=float(rng.choice([0.0, 0.01])), avoid_joint_limits_weight=float(rng.choice([0.0, 0.02])),
                  minimal_displacement_weight=float(rng.choice([0.001, 0.01])), cost_threshold=float(rng.choice([0.05, 1.0])))
    B = int(rng.integers(100, 125))
    o = O.Oracle(ch)
    goal, seed = problems(o, ch, rng, B, sigma=(1e-3, float(rng.choice([0.3, 1.0, 3.0]))))
    general = bool(M.general_step_pairs(ch)[0]) and family == "pik"
    model = M.Model(simds, kw["memetic_elite_size"], D, two_per_simd=2, general_dh_step=general)
    return o, Call(ch, kw, goal, seed, int(rng.integers(0, 1 << 62)), int(rng.integers(0, 1 << 40)), A_MARKS, model)


@pytest.mark.parametrize("D", range(1, 17))
@pytest.mark.parametrize("family", FAMILIES)
def test_every_chain_length_and_family(O, simds, family, D):
    o, c = family_call(O, family, D, simds)
    T = c.model.threshold
    s = pk.Solver(c.ch, device=0, exact=None if family == "pik_exact" else False)
    try:
        s.set_option("two_per_simd", "2")
        what = f"{family} D {D}"
        ref = reference(s, o, O, c, family, what)
        for load in (0, T, 10 * T):
            rec, ids = check_routed(s, c, load, ref, what)
            assert all(n >= 1 for n, _, _ in rec), rec  # (the unreachable fifth)
            if load == 0:
                assert all(pk.Solver.VARIANT_LANES[v] == c.model.widest() for v in ids[1:]), ids
                assert c.model.widest() == (4 if c.model.general_dh_step else 16)
            elif D <= 9:
                assert 7 in ids[1:] and 1 in ids[1:], (what, rec)
            else:
                assert 7 not in ids and set(ids[1:]) == {1}, (what, rec)
        host_rule(s, c, ref, what)
    finally:
        s.close()


# ---- b. elite group sizes ------------------------------------------------------------------------------------------

B_MARKS = (1, 3, 6, 10)


@pytest.mark.parametrize("exact", [False, None], ids=["fast", "exact"])
@pytest.mark.parametrize("D", [5, 11])
@pytest.mark.parametrize("elites", [1, 2, 3, 5, 8, 9, 16, 17, 32, 33, 64])
def test_every_elite_group_size(O, simds, elites, D, exact):
    rng = np.random.default_rng([0xB, elites, D])
    ch = random_chain(np.random.default_rng([0xB0B, D]), D)
    inside, close = M.general_step_pairs(ch)
    assert not close
    kw = dict(memetic_population_size=elites + 8, memetic_elite_size=elites, memetic_max_generations=12,
              memetic_gd_max_iters=int(rng.choice([5, 12])))
    o = O.Oracle(ch)
    goal, seed = problems(o, ch, rng, int(rng.integers(65, 100)))
    model = M.Model(simds, elites, D, two_per_simd=2, general_dh_step=bool(inside) and exact is False)
    c = Call(ch, kw, goal, seed, int(rng.integers(0, 1 << 62)), int(rng.integers(0, 1 << 40)), B_MARKS, model)
    gs = M.pow2ceil(elites)
    widest = {1: 16, 2: 16, 4: 16, 8: 8, 16: 4, 32: 2, 64: 1}[gs]
    assert model.widest() == (min(widest, 4) if model.general_dh_step else widest)
    s = pk.Solver(ch, device=0, exact=exact)
    try:
        s.set_option("two_per_simd", "2")
        what = f"elites {elites} D {D} exact {exact}"
        ref = reference(s, o, O, c, "pik" if exact is False else "pik_exact", what)
        for load in (0, 10 * model.threshold):
            rec, ids = check_routed(s, c, load, ref, what)
            assert all(n >= 1 for n, _, _ in rec), rec
            if load == 0:
                assert all(pk.Solver.VARIANT_LANES[v] == model.widest() for v in ids), ids
            else:
                assert all(pk.Solver.VARIANT_LANES[v] == 1 for v in ids[1:]), ids
        host_rule(s, c, ref, what)
    finally:
        s.close()


# ---- c. literal kernels behind a fast handle -----------------------------------------------------------------------

def mimic_panda():
    from tests.test_mimic_cpu import CASES, with_mimic
    name, k, master, mult, off = CASES[0]  # (a revolute joint of the Panda following another one)
    assert name == "panda"
    return with_mimic(np.random.default_rng(5 + k), robots.by_name(name), k, master, mult, off)[0]


@pytest.mark.parametrize("which", ["floating_panda", "mimic_panda", "panda_large_step"])
def test_literal_kernels_behind_a_fast_handle(O, simds, which):
    ch = {"floating_panda": robots.floating_panda, "mimic_panda": mimic_panda, "panda_large_step": robots.panda}[which]()
    rng = np.random.default_rng([0xC, ["floating_panda", "mimic_panda", "panda_large_step"].index(which)])
    kw = dict(memetic_population_size=24, memetic_max_generations=12, memetic_gd_max_iters=12)
    if which == "panda_large_step":
        kw["gd_step_size"] = 0.3
    assert ch.dof == {"floating_panda": 14, "mimic_panda": 6, "panda_large_step": 7}[which]
    o = O.Oracle(ch)
    goal, seed = problems(o, ch, rng, 90)
    # (the literal descent of a floating or a mimic joint has no two-per-SIMD build)
    model = M.Model(simds, 4, ch.dof, two_per_simd=2 if which == "panda_large_step" else 0)
    c = Call(ch, kw, goal, seed, 11, 3000, (1, 3, 6, 9), model)
    s = pk.Solver(ch, device=0, exact=False)
    try:
        s.set_option("two_per_simd", "2")
        ref = reference(s, o, O, c, "pik_exact", which)
        for load in (0, 10 * model.threshold):
            rec, ids = check_routed(s, c, load, ref, which)
            assert all(n >= 1 for n, _, _ in rec), rec
            assert all(pk.Solver.VARIANT_LANES[v] == (16 if load == 0 else 1) for v in ids[1:]), ids
        host_rule(s, c, ref, which)
    finally:
        s.close()


# ---- d. mark lists at the edges ------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def panda_pair(O):
    """an exact and a fast handle of the Panda, shared by the cases below (their slots keep what earlier calls left)"""
    hs = {None: pk.Solver(robots.panda(), device=0), False: pk.Solver(robots.panda(), device=0, exact=False)}
    for s in hs.values():
        s.set_option("two_per_simd", "2")
    yield hs
    for s in hs.values():
        s.close()


def panda_call(O, simds, rng_key, B, marks, generations=16, unreachable=None, sigma=(1e-3, 1.0), **more):
    ch = robots.panda()
    rng = np.random.default_rng([0xD, rng_key])
    kw = dict(memetic_population_size=32, memetic_max_generations=generations, memetic_gd_max_iters=12, **more)
    o = O.Oracle(ch)
    goal, seed = problems(o, ch, rng, B, unreachable, sigma)
    return o, Call(ch, kw, goal, seed, 1000 + rng_key, 77 * rng_key, marks, M.Model(simds, 4, 7, two_per_simd=2))


@pytest.mark.parametrize("exact", [None, False], ids=["exact", "fast"])
@pytest.mark.parametrize("marks,generations,n_records", [
    ((5,), 16, 2),
    (tuple(range(1, 16)), 16, 16),       # sixteen passes: every record, every per-pass counter of the slot
    ((3, 6, 10, 14, 200), 10, 3),        # marks at or above the budget are dropped
    ((16, 20, 31), 16, None),            # nothing left: one launch, no router
], ids=["one", "fifteen", "mixed", "none_left"])
def test_mark_lists_at_the_edges(O, simds, panda_pair, marks, generations, n_records, exact):
    o, c = panda_call(O, simds, len(marks), 90, marks, generations)
    s = panda_pair[exact]
    ns = "pik_exact" if exact is None else "pik_common"
    what = f"marks {marks} generations {generations} {ns}"
    ref = reference(s, o, O, c, ns, what)
    for load in (0, 10 * c.model.threshold):
        if n_records is None:
            got, rec = routed(s, c, load)
            assert rec is None and c.n_passes == 1, rec
            assert_same(got, ref, what)
            continue
        assert c.n_passes == n_records
        rec, ids = check_routed(s, c, load, ref, what)
        assert len(rec) == n_records and all(n >= 1 for n, _, _ in rec), rec
    host_rule(s, c, ref, what)


# ---- e. zero-survivor passes and slot re-use -----------------------------------------------------------------------

E_MARKS = (2, 4, 8, 12)
# the draw for which, by the oracle, some problems are still running at the marks 2 and 4 and every one has finished
# after five generations (found on the CPU among the draws 1..39, asserted below)
E_KEY = 14


def quick_call(O, simds):
    """reachable targets only, seeds close to a solution: every problem is done early"""
    return panda_call(O, simds, 100 + E_KEY, 70, E_MARKS, unreachable=0, sigma=(1e-3, 0.1),
                      stop_optimization_on_valid_solution=1)


def test_zero_survivor_passes_and_slot_reuse(O, simds):
    o, quick = quick_call(O, simds)
    _, large = panda_call(O, simds, 31, 150, E_MARKS)
    _, small = panda_call(O, simds, 32, 40, E_MARKS)
    with O.math_mode("fma"):
        refs = {id(c): o.solve_batch(c.params(O), c.goal, c.seed, rng_seed=c.rs, problem_offset=c.off,
                                     num_threads=O.max_threads()) for c in (quick, large, small)}
    gens = refs[id(quick)][3]["generations"]
    assert (refs[id(quick)][1] == pk.SUCCESS).all() and 4 < gens.max() < 8, gens.max()
    s = pk.Solver(robots.panda(), device=0)
    try:
        s.set_option("two_per_simd", "2")
        for load in (0, 10 * quick.model.threshold):
            for name, c in (("quick", quick), ("large", large), ("small", small), ("quick again", quick)):
                rec, ids = check_routed(s, c, load, refs[id(c)], f"{name} on a used slot")
                fresh = pk.Solver(robots.panda(), device=0)
                try:
                    fresh.set_option("two_per_simd", "2")
                    got, frec = routed(fresh, c, load)
                finally:
                    fresh.close()
                assert_same(got, refs[id(c)], f"{name} on a fresh handle")
                assert frec == rec, (name, frec, rec)
                if c is quick:
                    assert rec[1][0] >= 1 and rec[2][0] >= 1 and rec[3] == (0, load, 0) and rec[4] == (0, load, 0), rec
                else:
                    assert all(n >= 1 for n, _, _ in rec), rec
    finally:
        s.close()


# ---- f. load hygiene, g. real loads --------------------------------------------------------------------------------

def batch_of(c):
    return [(c.goal, c.seed, None, c.off)]


def as_job(s, c, job):
    s.set_option("device_regime", "1")
    s.set_option("lanes_per_elite", None)
    s.set_option("passes", c.passes())
    return s.solve_batches(c.params(), batch_of(c), rng_seed=c.rs, job=job)[0]


@pytest.mark.parametrize("exact", [None, False], ids=["exact", "fast"])
def test_a_finished_call_leaves_no_load_behind(O, simds, panda_pair, exact):
    s = panda_pair[exact]
    ns = "pik_exact" if exact is None else "pik_common"
    o, first = panda_call(O, simds, 41, 150, E_MARKS)
    _, second = panda_call(O, simds, 42, 100, E_MARKS)
    ref1, ref2 = reference(s, o, O, first, ns, "first"), reference(s, o, O, second, ns, "second")
    # a routed call as host job 0, waited for: its slot's load is back to 0 when another slot's routers look
    got = as_job(s, first, 0)
    s.wait(0)
    rec0 = s.debug_regime(pk.solver.MAX_SLOTS + 0)
    assert rec0 is not None and len(rec0) == first.n_passes and rec0[0][0] == first.B
    assert_same(got, ref1, "job 0")
    rec, _ = check_routed(s, second, 0, ref2, "after job 0")
    assert all(o_ == 0 for _, o_, _ in rec), rec
    # ... and a pool of batches as job 1
    cuts = [(0, 1), (1, 1), (1, 60), (60, first.B)]
    s.set_option("passes", first.passes())
    pooled = s.solve_batches(first.params(), [(first.goal[a:b], first.seed[a:b], None, first.off + a) for a, b in cuts],
                             rng_seed=first.rs, job=1)
    s.wait(1)
    rec1 = s.debug_regime(pk.solver.MAX_SLOTS + 1)
    assert rec1 is not None and rec1[0][0] == first.B
    for (a, b), g in zip(cuts, pooled):
        assert_same(g, [x[a:b] for x in ref1], f"pool batch {a}:{b}")
    rec, _ = check_routed(s, second, 0, ref2, "after the pool")
    assert all(o_ == 0 for _, o_, _ in rec), rec


def test_three_calls_in_flight_see_each_other(O, simds, panda_pair):
    s = panda_pair[None]
    o, quick = quick_call(O, simds)
    _, large = panda_call(O, simds, 51, 150, E_MARKS)
    _, middle = panda_call(O, simds, 52, 90, (1, 3, 5, 7, 9, 11))
    calls = (large, quick, middle)
    refs = [reference(s, o, O, c, "pik_exact", "alone") for c in calls]
    s.set_option("regime_threshold", "1")
    try:
        outs = [as_job(s, c, job) for job, c in enumerate(calls)]
        for job in range(3):
            s.wait(job)
        for job, (c, got, ref) in enumerate(zip(calls, outs, refs)):
            assert_same(got, ref, f"job {job}, three in flight")
            rec = s.debug_regime(pk.solver.MAX_SLOTS + job)
            assert rec is not None and len(rec) == c.n_passes and rec[0][0] == c.B, rec
            others = sum(x.B for x in calls) - c.B
            assert all(o_ <= others for _, o_, _ in rec), (rec, others)
            # (a load of at least 1 = the threshold: the throughput table; which passes saw one depends on timing)
            print(f"job {job}: {rec}; throughput regime in passes {[k for k, (_, o_, _) in enumerate(rec) if o_ >= 1]}")
            assert [v for _, _, v in rec[1:]] == [c.model.route(n, o_, 1) for n, o_, _ in rec[1:]], rec
        got, rec = routed(s, middle, 0)
        assert_same(got, refs[2], "after the three")
        assert rec is not None and all(o_ == 0 for _, o_, _ in rec), rec
    finally:
        s.set_option("regime_threshold", "")


# ---- h. a full pool ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("exact", [None, False], ids=["exact", "fast"])
@pytest.mark.parametrize("empty_ends", [False, True])
def test_a_full_pool_equals_its_single_calls(O, simds, panda_pair, empty_ends, exact):
    s = panda_pair[exact]
    rng = np.random.default_rng([0x8, int(empty_ends)])
    sizes = [int(x) for x in rng.choice([0, 1, 2, 3, 5, 7, 11, 13], size=pk.solver.MAX_BATCHES)]
    sizes[5], sizes[6], sizes[7] = 0, 1, 2
    if empty_ends:
        sizes[0] = sizes[-1] = 0
    else:
        sizes[0], sizes[-1] = 9, 1
    total = sum(sizes)
    assert len(sizes) == 64 and 200 <= total <= 400, total
    ch = robots.panda()
    o = O.Oracle(ch)
    kw = dict(memetic_population_size=24, memetic_max_generations=12, memetic_gd_max_iters=12)
    p = pk.default_params(**kw)
    goal, seed = problems(o, ch, rng, total)
    perm = rng.permutation(total)  # (the unreachable fifth spread over the batches)
    goal, seed = goal[perm], seed[perm]
    batches, a = [], 0
    for k, n in enumerate(sizes):
        batches.append((goal[a:a + n], seed[a:a + n], None, 1000 * k + 17))
        a += n
    model = M.Model(simds, 4, 7, two_per_simd=2)
    s.set_option("device_regime", "1")
    s.set_option("lanes_per_elite", None)
    s.set_option("passes", "1,3,6,9")
    singles = []
    for g, sd, _, off in batches:
        singles.append(s.solve_batch(p, g, sd, rng_seed=5, problem_offset=off))
        if len(g):
            rec = s.debug_regime(SYNC_SLOT)
            assert rec is not None and len(rec) == 5 and rec[0][0] == len(g), rec
    for load in (0, 10 * model.threshold):
        s.debug_regime(LOAD_SLOT, publish_load=load)
        try:
            pooled = s.solve_batches(p, batches, rng_seed=5)
        finally:
            rec = s.debug_regime(SYNC_SLOT)
            s.debug_regime(LOAD_SLOT, publish_load=0)
        print(f"pool of 64, {total} problems, load {load}: {rec}")
        assert rec is not None and len(rec) == 5
        model.check_record(rec, total, load)
        assert all(n >= 1 for n, _, _ in rec), rec
        for k, (got, single) in enumerate(zip(pooled, singles)):
            assert_same(got, single, f"batch {k} of {sizes[k]} load {load}")
    if exact is None:
        with O.math_mode("fma"):
            for k, (g, sd, _, off) in enumerate(batches):
                if len(g):
                    assert_same(singles[k], o.solve_batch(O.default_params(**kw), g, sd, rng_seed=5, problem_offset=off),
                                f"batch {k} against the oracle")


def test_device_entry_points_routed(simds):
    """a routed call on device slot 3 leaves no load behind, and a routed pool of HBM-resident batches fills its
    completion counters (own interpreter: torch allocates the buffers)"""
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "adaptive_device_check.py"), str(simds)],
                       cwd=ROOT,
                       capture_output=True, text=True, timeout=300)
    print(r.stdout[-3000:])
    assert r.returncode == 0 and "adaptive device check OK" in r.stdout, r.stdout[-2000:] + r.stderr[-3000:]
