"""Body of tests/test_gpu_startpath.py::test_device_entry_point_streams_and_slots (own interpreter: torch first, then
the library).  pikamd_search_paths_device on HBM-resident buffers and a non-default stream must equal the host-pointer
call bit for bit; two calls in flight on two slots and two streams must equal their serial answers."""
import sys

import numpy as np
import torch

torch.cuda.init()
sys.path.insert(0, ".")
import pick_ik_amd as pk  # noqa: E402
from pick_ik_amd.solver import STATS_DTYPE  # noqa: E402
from tests import startpath_reference as SP  # noqa: E402

dev = torch.device("cuda", 0)


class DeviceCall:
    """the arrays of one call in HBM"""

    def __init__(self, s, goals, seed, step):
        P, W = goals.shape[:2]
        self.P, self.W = P, W
        self.goals = torch.from_numpy(goals).to(dev)
        self.seed = torch.from_numpy(seed).to(dev)
        self.step = None if step is None else torch.from_numpy(step).to(dev)
        self.sol = torch.full((P, W, s.dof), -7.0, dtype=torch.float64, device=dev)
        self.st = torch.full((P, W), 77, dtype=torch.int32, device=dev)
        self.cost = torch.full((P, W), -7.0, dtype=torch.float64, device=dev)
        self.stats = torch.full((P, W, 3), -1, dtype=torch.int64, device=dev)
        self.reached = torch.full((P,), -1, dtype=torch.int32, device=dev)
        self.attempts = torch.full((P,), -1, dtype=torch.int32, device=dev)
        self.totals = torch.full((P, 3), -1, dtype=torch.int64, device=dev)

    def enqueue(self, s, p, K, stream, slot):
        s.search_paths_device(p, self.P, self.W, self.goals.data_ptr(), self.seed.data_ptr(), K, self.sol.data_ptr(),
                              self.st.data_ptr(), d_max_joint_step=0 if self.step is None else self.step.data_ptr(),
                              d_cost=self.cost.data_ptr(), d_stats=self.stats.data_ptr(), d_reached=self.reached.data_ptr(),
                              d_attempts=self.attempts.data_ptr(), d_totals=self.totals.data_ptr(), rng_seed=SP.RNG_SEED,
                              stream=stream.cuda_stream, slot=slot)

    def host(self):
        return (self.sol.cpu().numpy(), self.st.cpu().numpy(), self.cost.cpu().numpy(),
                self.stats.cpu().numpy().view(STATS_DTYPE).reshape(self.P, self.W), self.reached.cpu().numpy(),
                self.attempts.cpu().numpy(), self.totals.cpu().numpy().view(STATS_DTYPE).reshape(self.P))


def same(a, b, what):
    for x, y, w in zip(a, b, SP.NAMES):
        np.testing.assert_array_equal(x, y, err_msg=f"{what}: {w}")


assert STATS_DTYPE.itemsize == 24
for exact in (None, False):
    for case in ("panda", "torso_dual_arm"):
        ch = SP.CASES[case][0]()
        s = pk.Solver(ch, device=0, exact=exact)
        _, goals, seed, K, _ = SP.fixture(case, lambda c: s.fk)
        calls = [(pk.default_params(mode=1), None),
                 (pk.default_params(mode=1, minimal_displacement_weight=0.001), np.full(ch.dof, 0.15))]
        want = [s.search_paths(p, goals, seed, K, step, rng_seed=SP.RNG_SEED) for p, step in calls]
        assert (want[0][5] > 1).any() and (want[0][4] == goals.shape[1]).any()
        # (the host-pointer calls above carried the automatic self test; the stream-ordered entry point has none)
        streams = [torch.cuda.Stream(device=dev), torch.cuda.Stream(device=dev)]
        # one call on a stream of its own
        for (p, step), w in zip(calls, want):
            d = DeviceCall(s, goals, seed, step)
            torch.cuda.synchronize()
            with torch.cuda.stream(streams[0]):
                d.enqueue(s, p, K, streams[0], slot=5)
            streams[0].synchronize()
            same(d.host(), w, f"{case} exact={exact}: device call")
        # two calls with different parameters in flight on two slots and two streams, twice (the slots are reused)
        for rep in range(2):
            ds = [DeviceCall(s, goals, seed, step) for _, step in calls]
            torch.cuda.synchronize()
            for k in (0, 1):
                with torch.cuda.stream(streams[k]):
                    ds[k].enqueue(s, calls[k][0], K, streams[k], slot=2 + k)
            torch.cuda.synchronize()
            for k in (0, 1):
                same(ds[k].host(), want[k], f"{case} exact={exact}: slot {2 + k}, round {rep}")
        s.close()
print("startpath device check OK")
