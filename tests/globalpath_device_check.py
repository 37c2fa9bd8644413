"""Body of tests/test_gpu_globalpath.py::test_device_entry_point_streams_and_slots (own interpreter: torch first, then
the library).  pikamd_search_global_paths_device on HBM-resident buffers and a non-default stream must equal the
host-pointer call bit for bit -- it enqueues every attempt without a look at the open count --; two calls in flight on
two slots and two streams must equal their serial answers; and a second, smaller call on a slot that a larger one has
used must be right too (the slot's scratch does not shrink, and its pieces lie elsewhere in it)."""
import sys

import numpy as np
import torch

torch.cuda.init()
sys.path.insert(0, ".")
import pick_ik_amd as pk  # noqa: E402
from pick_ik_amd.solver import STATS_DTYPE  # noqa: E402
from tests import globalpath_reference as GP  # noqa: E402

dev = torch.device("cuda", 0)


class DeviceCall:
    """the arrays of one call in HBM"""

    def __init__(self, s, goals, seed, step):
        P, W = goals.shape[:2]
        self.P, self.W = P, W
        self.goals = torch.from_numpy(np.ascontiguousarray(goals)).to(dev)
        self.seed = torch.from_numpy(np.ascontiguousarray(seed)).to(dev)
        self.step = None if step is None else torch.from_numpy(step).to(dev)
        self.sol = torch.full((P, W, s.dof), -7.0, dtype=torch.float64, device=dev)
        self.st = torch.full((P, W), 77, dtype=torch.int32, device=dev)
        self.cost = torch.full((P, W), -7.0, dtype=torch.float64, device=dev)
        self.stats = torch.full((P, W, 3), -1, dtype=torch.int64, device=dev)
        self.reached = torch.full((P,), -1, dtype=torch.int32, device=dev)
        self.attempts = torch.full((P,), -1, dtype=torch.int32, device=dev)
        self.totals = torch.full((P, 3), -1, dtype=torch.int64, device=dev)

    def enqueue(self, s, p, K, stream, slot, problem_offset=0):
        s.search_global_paths_device(
            p, self.P, self.W, self.goals.data_ptr(), self.seed.data_ptr(), K, self.sol.data_ptr(), self.st.data_ptr(),
            d_max_joint_step=0 if self.step is None else self.step.data_ptr(), d_cost=self.cost.data_ptr(),
            d_stats=self.stats.data_ptr(), d_reached=self.reached.data_ptr(), d_attempts=self.attempts.data_ptr(),
            d_totals=self.totals.data_ptr(), rng_seed=GP.RNG_SEED, problem_offset=problem_offset,
            stream=stream.cuda_stream, slot=slot)

    def host(self):
        return (self.sol.cpu().numpy(), self.st.cpu().numpy(), self.cost.cpu().numpy(),
                self.stats.cpu().numpy().view(STATS_DTYPE).reshape(self.P, self.W), self.reached.cpu().numpy(),
                self.attempts.cpu().numpy(), self.totals.cpu().numpy().view(STATS_DTYPE).reshape(self.P))


def same(a, b, what):
    for x, y, w in zip(a, b, GP.NAMES):
        np.testing.assert_array_equal(x, y, err_msg=f"{what}: {w}")


assert STATS_DTYPE.itemsize == 24
case = "panda"
for exact in (None, False):
    s = pk.Solver(GP.SP.CASES[case][0](), device=0, exact=exact)
    ch, goals, seed, K, step = GP.fixture(case, lambda c: s.fk)
    calls = [(pk.default_params(**GP.params_kw(case)), None),
             (pk.default_params(**GP.params_kw(case, minimal_displacement_weight=0.001)), step)]
    want = [s.search_global_paths(p, goals, seed, K, st, rng_seed=GP.RNG_SEED) for p, st in calls]
    assert (want[0][5] > 1).any() and (want[0][4] == goals.shape[1]).any() and (want[0][4] < goals.shape[1]).any()
    # (the host-pointer calls above carried the automatic self tests; the stream-ordered entry point has none)
    streams = [torch.cuda.Stream(device=dev), torch.cuda.Stream(device=dev)]
    # one call on a stream of its own, then a smaller one on the same slot: paths 7.. of the call, keyed as such
    for (p, st), w in zip(calls, want):
        d = DeviceCall(s, goals, seed, st)
        small = DeviceCall(s, goals[7:20], seed[7:20], st)
        torch.cuda.synchronize()
        with torch.cuda.stream(streams[0]):
            d.enqueue(s, p, K, streams[0], slot=5)
            small.enqueue(s, p, K, streams[0], slot=5, problem_offset=7)
        streams[0].synchronize()
        same(d.host(), w, f"{case} exact={exact}: device call")
        same(small.host(), [x[7:20] for x in w], f"{case} exact={exact}: a smaller call behind it on the slot")
    # two calls with different parameters in flight on two slots and two streams, twice (the slots are reused)
    for rep in range(2):
        ds = [DeviceCall(s, goals, seed, st) for _, st in calls]
        torch.cuda.synchronize()
        for k in (0, 1):
            with torch.cuda.stream(streams[k]):
                ds[k].enqueue(s, calls[k][0], K, streams[k], slot=2 + k)
        torch.cuda.synchronize()
        for k in (0, 1):
            same(ds[k].host(), want[k], f"{case} exact={exact}: slot {2 + k}, round {rep}")
    s.close()
print("globalpath device check OK")
