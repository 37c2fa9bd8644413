"""Body of tests/test_gpu_polyline.py::test_device_entry_point_streams_and_slots (own interpreter: torch first, then
the library).  pikamd_cartesian_waypoints_device on HBM-resident buffers and a non-default stream must equal the
host-pointer call bit for bit -- with the poses returned and with the poses kept in the slot's scratch, a larger call
first and a smaller one on the same slot behind it (the scratch is reused, and the state of the larger call must not
show), then a slot that grows --; two calls in flight on two slots and two streams must equal their serial answers.
Behind the checks: the timing of one call against the host loop it replaces (measured, not asserted)."""
import sys

import numpy as np
import torch

torch.cuda.init()
sys.path.insert(0, ".")
import pick_ik_amd as pk  # noqa: E402
from pick_ik_amd import robots  # noqa: E402
from pick_ik_amd.solver import STATS_DTYPE  # noqa: E402
from tests import polyline_reference as LR  # noqa: E402

dev = torch.device("cuda", 0)
S, W = LR.S_POLYLINES, LR.W_POLYLINES


class DeviceCall:
    """the arrays of one call in HBM"""

    def __init__(self, s, start, targets, n_targets, step, with_goals):
        P = len(start)
        self.P = P
        self.start = torch.from_numpy(start).to(dev)
        self.targets = torch.from_numpy(np.ascontiguousarray(targets)).to(dev)
        self.count = torch.from_numpy(np.ascontiguousarray(n_targets)).to(dev)
        self.step = None if step is None else torch.from_numpy(step).to(dev)
        self.sol = torch.full((P, W, s.dof), -7.0, dtype=torch.float64, device=dev)
        self.st = torch.full((P, W), 77, dtype=torch.int32, device=dev)
        self.cost = torch.full((P, W), -7.0, dtype=torch.float64, device=dev)
        self.stats = torch.full((P, W, 3), -1, dtype=torch.int64, device=dev)
        self.reached = torch.full((P,), -1, dtype=torch.int32, device=dev)
        self.steps = torch.full((P,), -1, dtype=torch.int32, device=dev)
        self.segs = torch.full((P, S), -1, dtype=torch.int32, device=dev)
        self.fraction = torch.full((P,), -7.0, dtype=torch.float64, device=dev)
        self.goals = torch.full((P, W, 7), -7.0, dtype=torch.float64, device=dev) if with_goals else None

    def enqueue(self, s, p, c, stream, slot):
        s.cartesian_waypoints_device(
            p, c, self.P, S, W, self.start.data_ptr(), self.targets.data_ptr(), self.sol.data_ptr(), self.st.data_ptr(),
            self.steps.data_ptr(), d_n_targets=self.count.data_ptr(),
            d_max_joint_step=0 if self.step is None else self.step.data_ptr(), d_cost=self.cost.data_ptr(),
            d_stats=self.stats.data_ptr(), d_reached=self.reached.data_ptr(), d_segment_steps=self.segs.data_ptr(),
            d_fraction=self.fraction.data_ptr(), d_goals=0 if self.goals is None else self.goals.data_ptr(),
            stream=stream.cuda_stream, slot=slot)

    def host(self):
        """in the order of LR.NAMES, the poses left out when the call kept none"""
        out = [self.sol.cpu().numpy(), self.st.cpu().numpy(), self.cost.cpu().numpy(),
               self.stats.cpu().numpy().view(STATS_DTYPE).reshape(self.P, W), self.reached.cpu().numpy(),
               self.steps.cpu().numpy(), self.fraction.cpu().numpy(),
               None if self.goals is None else self.goals.cpu().numpy(), self.segs.cpu().numpy()]
        return out


def same(a, b, what):
    for x, y, w in zip(a, b, LR.NAMES):
        if x is not None:
            np.testing.assert_array_equal(x, y, err_msg=f"{what}: {w}")


for exact in (None, False):
    ch = robots.panda()
    s = pk.Solver(ch, device=0, exact=exact)
    start, targets, n_targets = LR.polylines(ch)
    c = pk.Cartesian(**LR.POLYLINES)
    calls = [(pk.default_params(mode=1), None),
             (pk.default_params(mode=1, minimal_displacement_weight=0.001), np.full(ch.dof, 0.1))]
    want = [s.cartesian_waypoints(p, c, start, targets, W, n_targets, step) for p, step in calls]
    small = [s.cartesian_waypoints(p, c, start[:9], targets[:9], W, n_targets[:9], step) for p, step in calls]
    # (the host-pointer calls above carried the automatic self test; the stream-ordered entry point has none)
    streams = [torch.cuda.Stream(device=dev), torch.cuda.Stream(device=dev)]
    # one call on a stream of its own.  Slot 5: the larger call, the smaller one behind it in the same scratch, the
    # poses returned; slot 6: the smaller call first, so that the larger one behind it grows the scratch
    for (p, step), w, ws in zip(calls, want, small):
        for slot, n, ww, with_goals in ((5, len(start), w, False), (5, 9, ws, False), (5, len(start), w, True),
                                        (6, 9, ws, False), (6, len(start), w, False)):
            d = DeviceCall(s, start[:n], targets[:n], n_targets[:n], step, with_goals)
            torch.cuda.synchronize()
            with torch.cuda.stream(streams[0]):
                d.enqueue(s, p, c, streams[0], slot=slot)
            streams[0].synchronize()
            same(d.host(), ww, f"exact={exact}: device call of {n} paths on slot {slot}, goals {with_goals}")
    # two calls with different parameters in flight on two slots and two streams, twice (the slots are reused)
    for rep in range(2):
        ds = [DeviceCall(s, start, targets, n_targets, step, rep == 1) for _, step in calls]
        torch.cuda.synchronize()
        for k in (0, 1):
            with torch.cuda.stream(streams[k]):
                ds[k].enqueue(s, calls[k][0], c, streams[k], slot=2 + k)
        torch.cuda.synchronize()
        for k in (0, 1):
            same(ds[k].host(), want[k], f"exact={exact}: slot {2 + k}, round {rep}")
    # timing, measured and not asserted: the call against S cartesian_paths calls with the host picking and repacking
    # the complete paths between them and the stitched relative test in numpy
    p = calls[0][0]
    tc, tl = LR.time_waypoints_against_host_loop(s, p, c, start, targets, W, n_targets)
    print(f"timing exact={exact} panda polylines (P = {len(start)}, S = {S}, W = {W}): call {tc * 1e3:.3f} ms, host loop {tl * 1e3:.3f} ms")
    tc, tl = LR.time_waypoints_against_host_loop(s, p, c, start[3:4], targets[3:4], W, n_targets[3:4])  # (three targets)
    print(f"timing exact={exact} one path (S = {S}, W = {W}): call {tc * 1e3:.3f} ms, host loop {tl * 1e3:.3f} ms")
    s.close()
print("polyline device check OK")
