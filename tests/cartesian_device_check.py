"""Body of tests/test_gpu_cartesian.py::test_device_entry_point_streams_and_slots (own interpreter: torch first, then
the library).  pikamd_cartesian_paths_device on HBM-resident buffers and a non-default stream must equal the
host-pointer call bit for bit -- with the poses returned and with the poses kept in the slot's scratch, a small call
first and a larger one on the same slot behind it, so that the scratch grows --; two calls in flight on two slots and
two streams must equal their serial answers."""
import sys

import numpy as np
import torch

torch.cuda.init()
sys.path.insert(0, ".")
import pick_ik_amd as pk  # noqa: E402
from pick_ik_amd import robots  # noqa: E402
from pick_ik_amd.solver import STATS_DTYPE  # noqa: E402
from tests import cartesian_reference as CR  # noqa: E402

dev = torch.device("cuda", 0)
W = 12
NAMES = CR.NAMES + ("goals",)


class DeviceCall:
    """the arrays of one call in HBM"""

    def __init__(self, s, start, target, step, with_goals):
        P = len(start)
        self.P = P
        self.start = torch.from_numpy(start).to(dev)
        self.target = torch.from_numpy(target).to(dev)
        self.step = None if step is None else torch.from_numpy(step).to(dev)
        self.sol = torch.full((P, W, s.dof), -7.0, dtype=torch.float64, device=dev)
        self.st = torch.full((P, W), 77, dtype=torch.int32, device=dev)
        self.cost = torch.full((P, W), -7.0, dtype=torch.float64, device=dev)
        self.stats = torch.full((P, W, 3), -1, dtype=torch.int64, device=dev)
        self.reached = torch.full((P,), -1, dtype=torch.int32, device=dev)
        self.steps = torch.full((P,), -1, dtype=torch.int32, device=dev)
        self.fraction = torch.full((P,), -7.0, dtype=torch.float64, device=dev)
        self.goals = torch.full((P, W, 7), -7.0, dtype=torch.float64, device=dev) if with_goals else None

    def enqueue(self, s, p, c, stream, slot):
        s.cartesian_paths_device(p, c, self.P, W, self.start.data_ptr(), self.target.data_ptr(), self.sol.data_ptr(),
                                 self.st.data_ptr(), self.steps.data_ptr(),
                                 d_max_joint_step=0 if self.step is None else self.step.data_ptr(),
                                 d_cost=self.cost.data_ptr(), d_stats=self.stats.data_ptr(), d_reached=self.reached.data_ptr(),
                                 d_fraction=self.fraction.data_ptr(), d_goals=0 if self.goals is None else self.goals.data_ptr(),
                                 stream=stream.cuda_stream, slot=slot)

    def host(self):
        out = (self.sol.cpu().numpy(), self.st.cpu().numpy(), self.cost.cpu().numpy(),
               self.stats.cpu().numpy().view(STATS_DTYPE).reshape(self.P, W), self.reached.cpu().numpy(),
               self.steps.cpu().numpy(), self.fraction.cpu().numpy())
        return out + ((self.goals.cpu().numpy(),) if self.goals is not None else ())


def same(a, b, what):
    for x, y, w in zip(a, b, NAMES):  # (a call without the poses: the seven arrays in front)
        np.testing.assert_array_equal(x, y, err_msg=f"{what}: {w}")


for exact in (None, False):
    ch = robots.panda()
    s = pk.Solver(ch, device=0, exact=exact)
    start, target = CR.offsets(ch)
    c = pk.Cartesian(**CR.OFFSETS)
    calls = [(pk.default_params(mode=1), None),
             (pk.default_params(mode=1, minimal_displacement_weight=0.001), np.full(ch.dof, 0.1))]
    want = [s.cartesian_paths(p, c, start, target, W, step) for p, step in calls]
    small = [s.cartesian_paths(p, c, start[:9], target[:9], W, step) for p, step in calls]
    # (the host-pointer calls above carried the automatic self test; the stream-ordered entry point has none)
    streams = [torch.cuda.Stream(device=dev), torch.cuda.Stream(device=dev)]
    # one call on a stream of its own: the poses in the slot's scratch -- a small call first, so that the larger one
    # behind it on the same slot grows the scratch --, then the poses returned
    for (p, step), w, ws in zip(calls, want, small):
        for n, ww, with_goals in ((9, ws, False), (len(start), w, False), (len(start), w, True)):
            d = DeviceCall(s, start[:n], target[:n], step, with_goals)
            torch.cuda.synchronize()
            with torch.cuda.stream(streams[0]):
                d.enqueue(s, p, c, streams[0], slot=5)
            streams[0].synchronize()
            same(d.host(), ww, f"exact={exact}: device call of {n} paths, goals {with_goals}")
    # two calls with different parameters in flight on two slots and two streams, twice (the slots are reused)
    for rep in range(2):
        ds = [DeviceCall(s, start, target, step, rep == 1) for _, step in calls]
        torch.cuda.synchronize()
        for k in (0, 1):
            with torch.cuda.stream(streams[k]):
                ds[k].enqueue(s, calls[k][0], c, streams[k], slot=2 + k)
        torch.cuda.synchronize()
        for k in (0, 1):
            same(ds[k].host(), want[k], f"exact={exact}: slot {2 + k}, round {rep}")
    s.close()
print("cartesian device check OK")
