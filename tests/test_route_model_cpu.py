"""tests/route_model.py, the plain model of the adaptive passes' range tables the GPU tests hold the routers' records
against (tests/test_gpu_adaptive_passes.py): it reproduces the rule tests/test_gpu_device_regime.py states for four
elites and seven variables, and tables written out by hand for the other elite group sizes and both sides of the
chain length at which the two-per-SIMD variant ends."""
import numpy as np
import pytest

from tests import route_model as M

S = 1024  # SIMDs of an MI355X
MAX = 0xFFFFFFFF


def test_model_reproduces_the_host_rule_for_four_elites_and_seven_variables():
    from tests.test_gpu_device_regime import host_variant, threshold
    for simds in (1024, 512, 304):
        m = M.Model(simds, 4, 7)
        assert m.widths == {16, 8, 4, 2} and m.threshold == threshold(simds)
        edges = [h + d for t in (m.latency, m.throughput) for _, _, h in t if h < MAX for d in (-1, 0, 1, 2)]
        sweep = sorted(set(range(0, 70)) | set(edges) | set(range(1, 40 * simds, 97)) | {MAX})
        for thr in (False, True):
            for n in sweep:
                assert m.host(n, thr) == host_variant(n, simds, thr), (simds, n, thr)
                load = m.threshold if thr else m.threshold - 1
                assert m.route(n, load) == host_variant(n, simds, thr), (simds, n, thr)
        assert m.route(0, 0) == 0 and m.route(0, 10 * m.threshold) == 0
        # the threshold is an argument of a decision, "at least" it
        assert m.route(9000, 5, threshold=5) == host_variant(9000, simds, True)
        assert m.route(9000, 4, threshold=5) == host_variant(9000, simds, False)


# (elites, D) -> latency table, throughput table; 1024 SIMDs, the library's default two_per_simd
HAND = {
    # gs = 1: 4 / 8 / 16 / 32 problems of 16 / 8 / 4 / 2 lanes in a wavefront; 1152 * 64 - 1 and 640 * 64 - 1
    (1, 9): ([(5, 0, 4096), (4, 4096, 8192), (3, 8192, 16384), (2, 16384, 32768), (1, 32768, 73727), (7, 73727, MAX)],
             [(1, 0, 40959), (7, 40959, MAX)]),
    (1, 10): ([(5, 0, 4096), (4, 4096, 8192), (3, 8192, 16384), (2, 16384, 32768), (1, 32768, MAX)],
              [(1, 0, MAX)]),
    # gs = 8: no 16 lanes (128 > 64); 1152 * 8 - 1 and 640 * 8 - 1
    (8, 9): ([(4, 0, 1024), (3, 1024, 2048), (2, 2048, 4096), (1, 4096, 9215), (7, 9215, MAX)],
             [(1, 0, 5119), (7, 5119, MAX)]),
    (8, 10): ([(4, 0, 1024), (3, 1024, 2048), (2, 2048, 4096), (1, 4096, MAX)], [(1, 0, MAX)]),
    (5, 9): ([(4, 0, 1024), (3, 1024, 2048), (2, 2048, 4096), (1, 4096, 9215), (7, 9215, MAX)],
             [(1, 0, 5119), (7, 5119, MAX)]),
    # gs = 16
    (16, 9): ([(3, 0, 1024), (2, 1024, 2048), (1, 2048, 4607), (7, 4607, MAX)], [(1, 0, 2559), (7, 2559, MAX)]),
    (16, 10): ([(3, 0, 1024), (2, 1024, 2048), (1, 2048, MAX)], [(1, 0, MAX)]),
    # gs = 32
    (32, 9): ([(2, 0, 1024), (1, 1024, 2303), (7, 2303, MAX)], [(1, 0, 1279), (7, 1279, MAX)]),
    (17, 10): ([(2, 0, 1024), (1, 1024, MAX)], [(1, 0, MAX)]),
    # gs = 64: one lane per elite fills the wavefront
    (64, 9): ([(1, 0, 1151), (7, 1151, MAX)], [(1, 0, 639), (7, 639, MAX)]),
    (33, 10): ([(1, 0, MAX)], [(1, 0, MAX)]),
}


@pytest.mark.parametrize("elites,D", sorted(HAND))
def test_hand_written_tables(elites, D):
    m = M.Model(S, elites, D)
    lat, thr = HAND[(elites, D)]
    assert m.latency == lat and m.throughput == thr
    assert m.threshold == S * 64 // M.pow2ceil(elites) // 2
    # the decisions at every edge of both tables
    for tab, load in ((lat, 0), (thr, m.threshold)):
        for vid, lo, hi in tab:
            assert m.route(hi, load) == vid and m.route(lo + 1, load) == vid
            if lo > 0:
                assert m.route(lo, load) != vid
    assert m.route(0, 0) == 0 and m.route(0, m.threshold) == 0
    assert m.widest() == max([pk_lanes(v) for v, _, _ in lat])


def pk_lanes(vid):
    import pick_ik_amd as pk
    return pk.Solver.VARIANT_LANES[vid]


def test_two_per_simd_option_and_restricted_widths():
    # an explicit threshold (first-pass wavefronts) holds in both regimes: the one-per-SIMD build up to 2 * 64 / gs - 1
    m = M.Model(S, 4, 9, two_per_simd=2)
    assert m.latency == [(5, 0, 1024), (4, 1024, 2048), (3, 2048, 4096), (2, 4096, 8192), (1, 8192, 8192), (7, 8192, MAX)]
    assert m.throughput == [(1, 0, 31), (7, 31, MAX)]
    assert m.route(8193, 0) == 7 and m.route(8192, 0) == 2  # (the empty range of variant 1 is never chosen)
    assert [m.route(n, m.threshold) for n in (1, 31, 32, 160)] == [1, 1, 7, 7]
    m = M.Model(S, 64, 5, two_per_simd=2)
    assert m.latency == m.throughput == [(1, 0, 1), (7, 1, MAX)]
    m = M.Model(S, 4, 10, two_per_simd=2)  # ten variables: no two-per-SIMD variant whatever the option says
    assert m.throughput == [(1, 0, MAX)] and m.latency[-1] == (1, 8192, MAX)
    for v in (0, "0"):
        m = M.Model(S, 4, 7, two_per_simd=v)
        assert m.throughput == [(1, 0, MAX)] and m.latency[-1] == (1, 8192, MAX)
    m = M.Model(S, 4, 7, two_per_simd=1)  # (1: the default thresholds)
    assert (m.latency, m.throughput) == (M.Model(S, 4, 7).latency, M.Model(S, 4, 7).throughput)
    # a chain with a general Denavit-Hartenberg step on a fast handle: no cooperative descent
    m = M.Model(S, 4, 6, general_dh_step=True)
    assert m.widths == {4, 2} and m.latency[:2] == [(3, 0, 4096), (2, 4096, 8192)]
    assert M.Model(S, 16, 6, general_dh_step=True).widths == {4, 2}
    assert [M.pow2ceil(e) for e in (1, 2, 3, 4, 5, 8, 9, 16, 17, 32, 33, 64)] == [1, 2, 4, 4, 8, 8, 16, 16, 32, 32, 64, 64]


def test_check_record():
    m = M.Model(S, 4, 7, two_per_simd=2)
    T = m.threshold
    assert m.check_record([(100, T, 5), (40, T, 7), (20, T, 1), (0, T, 0)], 100, T) == [5, 7, 1, 0]
    for bad in ([(100, T, 5), (40, T, 1)], [(100, 0, 5), (40, T, 7)], [(99, T, 5)], [(100, T, 5), (0, T, 1)]):
        with pytest.raises(AssertionError):
            m.check_record(bad, 100, T)


def test_general_step_window_of_a_chain():
    import dataclasses
    from pick_ik_amd import robots
    ur5 = robots.ur5()
    assert M.general_step_pairs(ur5) == ([], [])
    for eps, want in ((1e-4, [1]), (4.9e-12, [1]), (0.2, [])):
        origin = ur5.origin_xyz_rpy.copy()
        origin[2, 3] += eps  # (the elbow tilted against the parallel lift axis: tests/test_gpu_fuzz.py)
        assert M.general_step_pairs(dataclasses.replace(ur5, origin_xyz_rpy=origin))[0] == want, eps
    assert M.general_step_pairs(robots.panda()) == ([], [])


def test_general_family_has_unbounded_variables_and_plain_steps():
    from pick_ik_amd import robots
    from tests.test_gpu_adaptive_passes import FAMILIES, family_chain
    chains = [family_chain("pik", D) for D in range(1, 17)]
    assert sum(bool((np.asarray(ch.bounded) == 0).any()) for ch in chains) >= 4
    kinds = set(int(t) for ch in chains for t in ch.joint_type)
    assert {robots.REVOLUTE, robots.PRISMATIC, robots.PLANAR_X} <= kinds
    for family in FAMILIES[:3]:  # (what the model is told about the fast families' chains is decidable)
        for D in range(1, 17):
            inside, close = M.general_step_pairs(family_chain(family, D))
            assert not close and (family == "pik" or not inside), (family, D, inside, close)
    assert M.general_step_pairs(family_chain("pik", 15))[0] == [2]  # (the restricted widths are covered)
