"""The routed launcher (option device_regime, pick_ik_amd/csrc/pik_route.hpp): the regime of every compaction pass --
latency or throughput schedule -- is chosen by a router kernel when the pass starts, from the load the other slots
publish.  A scheduling choice: every setting must give the same bits, and the record the routers leave
(pikamd_debug_regime) must show the host's range tables applied to the survivor counts.

Set-up of every case: Panda, population 128, four elites, 100 generations, B = 1.5 x the problems that get a
16-lane wavefront each in one round (1536 on 256 CUs: the smallest call that is cut into passes), the last 64 targets
out of reach, so that every pass has survivors."""
import numpy as np
import pytest

import pick_ik_amd as pk
from pick_ik_amd import robots

pytestmark = pytest.mark.gpu

GS = 4  # pow2ceil(elites)
SYNC_SLOT = pk.solver.MAX_SLOTS + pk.solver.MAX_HOST_JOBS - 1  # the slot of the synchronous host-pointer calls
LOAD_SLOT = 5  # a device slot no call of this file uses: carries the artificial load
KW = dict(memetic_population_size=128, memetic_elite_size=4, memetic_max_generations=100)
DEFAULT_MARKS = (2, 4, 8, 12, 16, 24, 32, 40, 48, 64, 80)


@pytest.fixture(scope="module")
def simds():
    """SIMDs of the first GPU, from the driver's topology files (no second runtime in this process)"""
    import glob
    for f in sorted(glob.glob("/sys/class/kfd/kfd/topology/nodes/*/properties"),
                    key=lambda f: int(f.split("/")[-2])):
        try:
            props = dict(line.split()[:2] for line in open(f) if len(line.split()) >= 2)
        except OSError:  # (another GPU of the box, not this process's)
            continue
        if int(props.get("simd_count", 0)) > 0:
            return int(props["simd_count"])
    pytest.fail("no GPU node in /sys/class/kfd/kfd/topology")


@pytest.fixture(scope="module", params=[None, False], ids=["exact", "fast"])
def panda(request):
    import __graft_entry__ as g
    g.build()
    s = pk.Solver(robots.panda(), device=0, exact=request.param)
    yield s
    s.close()


@pytest.fixture(scope="module")
def problem(simds):
    """(goal, seed): B targets, the last 64 pushed 1.0-1.5 m out along their own direction (bench.py --config 4)"""
    B = simds * 64 // (GS * 16) * 3 // 2
    ch = robots.panda()
    rng = np.random.default_rng(0xD0E)
    s = pk.Solver(ch, device=0)
    goal = s.fk(rng.uniform(ch.qmin, ch.qmax, size=(B, ch.dof)))
    s.close()
    d = goal[-64:, :3] / np.linalg.norm(goal[-64:, :3], axis=1, keepdims=True)
    goal[-64:, :3] = d * rng.uniform(1.0, 1.5, size=(64, 1))
    return goal, np.tile(robots.PANDA_HOME, (B, 1))


def threshold(simds):
    """the routers' default threshold: half of the problems that give every SIMD a one-lane wavefront"""
    return simds * 64 // GS // 2


def host_variant(n, simds, throughput):
    """launch_solve's adaptive rule for a pass of n problems on one tip frame with four elites: the variant id"""
    if n == 0:
        return 0
    if not throughput:
        for lanes, vid in ((16, 5), (8, 4), (4, 3), (2, 2)):
            if n <= simds * (64 // (GS * lanes)):
                return vid
    occ2_from = (simds * 5 // 8 if throughput else simds * 9 // 8) * 64 // GS
    return 1 if n <= occ2_from - 1 else 7


def assert_same(a, b, what):
    for x, y, w in zip(a, b, ("solution", "status", "cost", "stats")):
        np.testing.assert_array_equal(x, y, err_msg=f"{what}: {w}")


def solve(s, problem, **kw):
    goal, seed = problem
    return s.solve_batch(pk.default_params(**KW), goal, seed, rng_seed=77, **kw)


@pytest.fixture(scope="module")
def reference(panda, problem):
    """the host rule's answers (device_regime = 0), computed once"""
    panda.set_option("device_regime", "0")
    ref = solve(panda, problem)
    assert panda.debug_regime(SYNC_SLOT) is None
    panda.set_option("device_regime", "1")
    st = ref[1]
    assert (st[:-64] == pk.SUCCESS).mean() > 0.9 and (st[-64:] != pk.SUCCESS).any()  # (long runners to the last pass)
    return ref


def test_same_answers_and_routing_under_every_load(panda, problem, reference, simds, monkeypatch):
    s, T = panda, threshold(simds)
    records = {}
    for load in (0, T - 1, T, 10 * T):
        s.debug_regime(LOAD_SLOT, publish_load=load)
        try:
            got = solve(s, problem)
        finally:
            rec = s.debug_regime(SYNC_SLOT)
            s.debug_regime(LOAD_SLOT, publish_load=0)
        assert_same(got, reference, f"load {load}")
        assert rec is not None and len(rec) == len(DEFAULT_MARKS) + 1, rec
        print(f"load {load}: (survivors, others' load, variant) per pass = {rec}")
        records[load] = rec
        assert all(o == load for _, o, _ in rec), rec
        assert rec[0][0] == len(problem[0])
        assert all(n >= 1 for n, _, _ in rec) and all(rec[k][0] >= rec[k + 1][0] for k in range(len(rec) - 1))
    # nothing else in flight: the host's adaptive (latency) rule on the survivor counts; pass 0 is the host's choice
    for load in (0, T - 1):
        assert [v for _, _, v in records[load]] == [host_variant(n, simds, False) for n, _, _ in records[load]]
    assert records[T - 1] == [(n, T - 1, v) for n, _, v in records[0]]
    assert any(pk.Solver.VARIANT_LANES[v] > 1 for _, _, v in records[0][1:])
    # the others fill the chip: every routed pass (1 ..) one lane per elite, by the throughput table
    for load in (T, 10 * T):
        assert [v for _, _, v in records[load][1:]] == [host_variant(n, simds, True) for n, _, _ in records[load][1:]]
        assert all(pk.Solver.VARIANT_LANES[v] == 1 for _, _, v in records[load][1:])
    # ... and the forced regimes (launch_solve serves them)
    for regime in ("latency", "throughput"):
        monkeypatch.setenv("PIK_REGIME", regime)
        assert_same(solve(s, problem), reference, f"regime {regime}")
        assert s.debug_regime(SYNC_SLOT) is None
    monkeypatch.delenv("PIK_REGIME")
    assert_same(solve(s, problem), reference, "adaptive again")
    assert s.debug_regime(SYNC_SLOT) is not None


def test_regime_threshold_option_moves_the_switch(panda, problem, reference, simds):
    s, T = panda, threshold(simds)
    s.set_option("regime_threshold", str(2 * T))
    s.debug_regime(LOAD_SLOT, publish_load=T)
    try:
        got = solve(s, problem)
        rec = s.debug_regime(SYNC_SLOT)
    finally:
        s.debug_regime(LOAD_SLOT, publish_load=0)
        s.set_option("regime_threshold", "")
    assert_same(got, reference, "threshold 2 T, load T")
    assert [v for _, _, v in rec] == [host_variant(n, simds, False) for n, _, _ in rec]


def test_option_values(panda):
    for good in ("0", "1", ""):
        panda.set_option("device_regime", good)
    for bad in ("2", "-1", "on", "01", "1 ", "adaptive"):
        with pytest.raises(pk.PickIkAmdError, match="device_regime"):
            panda.set_option("device_regime", bad)
    with pytest.raises(pk.PickIkAmdError, match="regime_threshold"):
        panda.set_option("regime_threshold", "-3")


def test_ragged_pool_equals_single_calls(panda, problem, reference):
    s = panda
    goal, seed = problem
    B = len(goal)
    cuts = [(0, 1000), (1000, 1000), (1000, B)]  # (the second batch is empty)
    batches = [(goal[a:b], seed[a:b], None, a) for a, b in cuts]
    pooled = s.solve_batches(pk.default_params(**KW), batches, rng_seed=77)
    assert s.debug_regime(SYNC_SLOT) is not None
    for (a, b), got in zip(cuts, pooled):
        single = s.solve_batch(pk.default_params(**KW), goal[a:b], seed[a:b], rng_seed=77, problem_offset=a)
        assert_same(got, single, f"batch {a}:{b}")
        assert_same(got, [x[a:b] for x in reference], f"batch {a}:{b} against the whole call")


def test_same_call_twice_on_one_slot(panda, problem, reference):
    for rep in range(2):
        assert_same(solve(panda, problem), reference, f"repetition {rep}")
        assert panda.debug_regime(SYNC_SLOT) is not None


def test_two_calls_at_once_equal_one_after_the_other(panda, problem, reference):
    s = panda
    goal, seed = problem
    p = pk.default_params(**KW)
    a = [(goal, seed, None, 0)]
    b = [(goal[::-1].copy(), seed, None, 5000)]
    ra = s.solve_batches(p, a, rng_seed=77)
    rb = s.solve_batches(p, b, rng_seed=78)
    assert_same(ra[0], reference, "first call alone")
    ja = s.solve_batches(p, a, rng_seed=77, job=0)
    jb = s.solve_batches(p, b, rng_seed=78, job=1)
    s.wait(0)
    s.wait(1)
    assert_same(ja[0], ra[0], "first call, both in flight")
    assert_same(jb[0], rb[0], "second call, both in flight")
    for job in (0, 1):
        rec = s.debug_regime(pk.solver.MAX_SLOTS + job)
        assert rec is not None and len(rec) == len(DEFAULT_MARKS) + 1
        print(f"job {job}: {rec}")


def test_ineligible_calls_take_the_host_rule(panda, problem, reference, monkeypatch):
    s = panda
    goal, seed = problem
    # a forced schedule
    monkeypatch.setenv("PIK_LPE_SCHED", "0:1,16:4")
    assert_same(solve(s, problem), reference, "forced schedule")
    assert s.debug_regime(SYNC_SLOT) is None
    monkeypatch.delenv("PIK_LPE_SCHED")
    monkeypatch.setenv("PIK_LPE", "2")
    assert_same(solve(s, problem), reference, "forced lanes")
    assert s.debug_regime(SYNC_SLOT) is None
    monkeypatch.delenv("PIK_LPE")
    # two species
    s.solve_batch(pk.default_params(memetic_num_threads=2, **KW), goal[:1200], seed[:1200], rng_seed=77)
    assert s.debug_regime(SYNC_SLOT) is None
    # a call without passes
    s.solve_batch(pk.default_params(**KW), goal[:512], seed[:512], rng_seed=77)
    assert s.debug_regime(SYNC_SLOT) is None
    # two tip frames
    ch = robots.torso_dual_arm()
    m = pk.Solver(ch, device=0, exact=s.exact)
    rng = np.random.default_rng(5)
    g2 = m.fk(rng.uniform(ch.qmin, ch.qmax, size=(1200, ch.dof))).reshape(1200, -1)
    sd = np.clip(np.zeros((1200, ch.dof)), ch.qmin, ch.qmax)
    m.solve_batch(pk.default_params(memetic_population_size=32, memetic_max_generations=20), g2, sd, rng_seed=1)
    assert m.debug_regime(SYNC_SLOT) is None
    m.close()
    assert_same(solve(s, problem), reference, "routed again")
    assert s.debug_regime(SYNC_SLOT) is not None
