"""Body of tests/test_gpu_search.py::test_device_entry_point_streams_and_slots (own interpreter: torch first, then the
library).  pikamd_search_batch_device on HBM-resident buffers and a non-default stream must equal the host-pointer
call bit for bit, in both schedules; two calls in flight on two slots and two streams must equal their serial
answers."""
import sys

import numpy as np
import torch

torch.cuda.init()
sys.path.insert(0, ".")
import pick_ik_amd as pk  # noqa: E402
from pick_ik_amd.solver import STATS_DTYPE  # noqa: E402
from tests import search_reference as SR  # noqa: E402

dev = torch.device("cuda", 0)
B, K = 64, 4


class DeviceSearch:
    """the arrays of one search call in HBM"""

    def __init__(self, s, goals, seed, every):
        self.goals = torch.from_numpy(goals).to(dev)
        self.seed = torch.from_numpy(seed).to(dev)
        self.sol = torch.full((B, s.dof), -7.0, dtype=torch.float64, device=dev)
        self.st = torch.full((B,), 77, dtype=torch.int32, device=dev)
        self.cost = torch.full((B,), -7.0, dtype=torch.float64, device=dev)
        self.stats = torch.full((B, 3), -1, dtype=torch.int64, device=dev)
        self.attempts = torch.full((B,), -1, dtype=torch.int32, device=dev)
        self.all_sol = torch.full((B, K, s.dof), -7.0, dtype=torch.float64, device=dev) if every else None
        self.all_st = torch.full((B, K), 77, dtype=torch.int32, device=dev) if every else None

    def enqueue(self, s, p, rng_seed, stream, slot):
        s.search_batch_device(p, B, self.goals.data_ptr(), self.seed.data_ptr(), K, self.sol.data_ptr(),
                              self.st.data_ptr(), d_cost=self.cost.data_ptr(), d_stats=self.stats.data_ptr(),
                              d_attempts=self.attempts.data_ptr(),
                              d_all_solution=0 if self.all_sol is None else self.all_sol.data_ptr(),
                              d_all_status=0 if self.all_st is None else self.all_st.data_ptr(), rng_seed=rng_seed,
                              stream=stream.cuda_stream, slot=slot)

    def host(self):
        out = (self.sol.cpu().numpy(), self.st.cpu().numpy(), self.cost.cpu().numpy(),
               self.stats.cpu().numpy().view(STATS_DTYPE).reshape(B), self.attempts.cpu().numpy())
        if self.all_sol is not None:
            out += (self.all_sol.cpu().numpy(), self.all_st.cpu().numpy())
        return out


def same(a, b, what):
    assert len(a) == len(b)
    for x, y, w in zip(a, b, SR.NAMES + ("all_solution", "all_status")):
        np.testing.assert_array_equal(x, y, err_msg=f"{what}: {w}")


for exact in (None, False):
    for case in ("panda", "torso_dual_arm"):
        s = pk.Solver(SR.CASES[case][0](), device=0, exact=exact)
        ch, goals, seed, kw = SR.fixture(case, lambda _: s.fk, B)
        # (parameters, rng_seed, every attempt wanted)
        calls = [(pk.default_params(mode=1), 0, False),
                 (pk.default_params(mode=1, minimal_displacement_weight=0.001), 9, True)]
        want = [s.search_batch(p, goals, seed, K, rng_seed=r, all_attempts=e) for p, r, e in calls]
        first, later, never = SR.search_counts(want[0][1], want[0][4])
        assert first >= 1 and later >= 1, (first, later, never)
        # (the host-pointer calls above carried the automatic self test; the stream-ordered entry point has none)
        streams = [torch.cuda.Stream(device=dev), torch.cuda.Stream(device=dev)]
        for schedule in ("sequential", "parallel"):
            s.set_option("search_schedule", schedule)
            # one call on a stream of its own
            for (p, r, e), w in zip(calls, want):
                d = DeviceSearch(s, goals, seed, e)
                torch.cuda.synchronize()
                with torch.cuda.stream(streams[0]):
                    d.enqueue(s, p, r, streams[0], slot=5)
                streams[0].synchronize()
                same(d.host(), w, f"{case} exact={exact} {schedule}: device call")
            # two calls with different parameters in flight on two slots and two streams, twice (the slots are reused)
            for rep in range(2):
                ds = [DeviceSearch(s, goals, seed, e) for _, _, e in calls]
                torch.cuda.synchronize()
                for k in (0, 1):
                    with torch.cuda.stream(streams[k]):
                        ds[k].enqueue(s, calls[k][0], calls[k][1], streams[k], slot=2 + k)
                torch.cuda.synchronize()
                for k in (0, 1):
                    same(ds[k].host(), want[k], f"{case} exact={exact} {schedule}: slot {2 + k}, round {rep}")
        s.close()
print("search device check OK")
