"""Body of tests/test_gpu_search_global.py::test_device_entry_point_streams_and_slots (own interpreter: torch first, then
the library).  pikamd_search_global_batch_device on HBM-resident buffers and a non-default stream must equal the
host-pointer call bit for bit; two calls in flight on two slots and two streams must equal their serial answers; one
slot serves a larger, then a smaller call, then the first one again."""
import sys

import numpy as np
import torch

torch.cuda.init()
sys.path.insert(0, ".")
import pick_ik_amd as pk  # noqa: E402
from pick_ik_amd.solver import STATS_DTYPE  # noqa: E402
from tests import search_global_reference as GR  # noqa: E402
from tests import search_reference as SR  # noqa: E402

dev = torch.device("cuda", 0)
K = GR.K


class DeviceSearch:
    """the arrays of one search call in HBM"""

    def __init__(self, s, goals, seed, every):
        self.n = n = len(seed)
        self.goals = torch.from_numpy(np.ascontiguousarray(goals)).to(dev)
        self.seed = torch.from_numpy(np.ascontiguousarray(seed)).to(dev)
        self.sol = torch.full((n, s.dof), -7.0, dtype=torch.float64, device=dev)
        self.st = torch.full((n,), 77, dtype=torch.int32, device=dev)
        self.cost = torch.full((n,), -7.0, dtype=torch.float64, device=dev)
        self.stats = torch.full((n, 3), -1, dtype=torch.int64, device=dev)
        self.attempts = torch.full((n,), -1, dtype=torch.int32, device=dev)
        self.all_sol = torch.full((n, K, s.dof), -7.0, dtype=torch.float64, device=dev) if every else None
        self.all_st = torch.full((n, K), 77, dtype=torch.int32, device=dev) if every else None

    def enqueue(self, s, p, rng_seed, stream, slot):
        s.search_global_batch_device(p, self.n, self.goals.data_ptr(), self.seed.data_ptr(), K, self.sol.data_ptr(),
                                     self.st.data_ptr(), d_cost=self.cost.data_ptr(), d_stats=self.stats.data_ptr(),
                                     d_attempts=self.attempts.data_ptr(),
                                     d_all_solution=0 if self.all_sol is None else self.all_sol.data_ptr(),
                                     d_all_status=0 if self.all_st is None else self.all_st.data_ptr(),
                                     rng_seed=rng_seed, stream=stream.cuda_stream, slot=slot)

    def host(self):
        out = (self.sol.cpu().numpy(), self.st.cpu().numpy(), self.cost.cpu().numpy(),
               self.stats.cpu().numpy().view(STATS_DTYPE).reshape(self.n), self.attempts.cpu().numpy())
        if self.all_sol is not None:
            out += (self.all_sol.cpu().numpy(), self.all_st.cpu().numpy())
        return out


def same(a, b, what):
    assert len(a) == len(b)
    for x, y, w in zip(a, b, SR.NAMES + ("all_solution", "all_status")):
        np.testing.assert_array_equal(x, y, err_msg=f"{what}: {w}")


for exact, case, B in ((None, "panda", 64), (False, "panda", 64), (False, "torso_dual_arm", 64), (None, "panda", 600)):
    s = pk.Solver(SR.CASES[case][0](), device=0, exact=exact)
    ch, goals, seed = GR.fixture(case, lambda _: s.fk, B)
    # (parameters, rng_seed, every attempt wanted)
    calls = [(pk.default_params(mode=0, **GR.params_kw(case)), 1, False),
             (pk.default_params(mode=0, **GR.params_kw(case, minimal_displacement_weight=0.001)), 9, True)]
    want = [s.search_global_batch(p, goals, seed, K, rng_seed=r, all_attempts=e) for p, r, e in calls]
    first, later, never = SR.search_counts(want[0][1], want[0][4])
    assert later >= 1 and never >= 1, (first, later, never)
    # (the host-pointer calls above carried the automatic self test; the stream-ordered entry point has none)
    streams = [torch.cuda.Stream(device=dev), torch.cuda.Stream(device=dev)]
    # one call on a stream of its own
    for (p, r, e), w in zip(calls, want):
        d = DeviceSearch(s, goals, seed, e)
        torch.cuda.synchronize()
        with torch.cuda.stream(streams[0]):
            d.enqueue(s, p, r, streams[0], slot=5)
        streams[0].synchronize()
        same(d.host(), w, f"{case} exact={exact} B={B}: device call")
    # two calls with different parameters in flight on two slots and two streams, twice (the slots are reused)
    for rep in range(2):
        ds = [DeviceSearch(s, goals, seed, e) for _, _, e in calls]
        torch.cuda.synchronize()
        for k in (0, 1):
            with torch.cuda.stream(streams[k]):
                ds[k].enqueue(s, calls[k][0], calls[k][1], streams[k], slot=2 + k)
        torch.cuda.synchronize()
        for k in (0, 1):
            same(ds[k].host(), want[k], f"{case} exact={exact} B={B}: slot {2 + k}, round {rep}")
    # the stream-ordered call does not know how many problems an attempt has: every reachable variant is enqueued
    # and the device-side count picks one -- under forced schedules too
    for name, value in (("passes", "2,4,8"), ("lanes_per_elite", "1"), ("lanes_per_elite", "4"), ("regime", "throughput"),
                        ("two_per_simd", "2"), ("device_regime", "0")):
        s.set_option(name, value)
        for (p, r, e), w in zip(calls, want):
            d = DeviceSearch(s, goals, seed, e)
            torch.cuda.synchronize()
            with torch.cuda.stream(streams[0]):
                d.enqueue(s, p, r, streams[0], slot=4)
            streams[0].synchronize()
            same(d.host(), w, f"{case} exact={exact} B={B}: device call, {name} = {value}")
        s.set_option(name, None)
    # a larger call, a smaller one and the first again on ONE slot (its scratch grows once and is reused)
    p, r, e = calls[0]
    n_small = 5
    small = s.search_global_batch(p, goals[B - n_small:], seed[B - n_small:], K, rng_seed=r)
    for what, g, sd, w in (("larger", goals, seed, want[0]), ("smaller", goals[B - n_small:], seed[B - n_small:], small),
                           ("larger again", goals, seed, want[0])):
        d = DeviceSearch(s, g, sd, e)
        torch.cuda.synchronize()
        with torch.cuda.stream(streams[1]):
            d.enqueue(s, p, r, streams[1], slot=6)
        streams[1].synchronize()
        same(d.host(), w, f"{case} exact={exact} B={B}: {what} on slot 6")
    s.close()
print("search global device check OK")
