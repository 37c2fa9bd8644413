"""Body of tests/test_gpu_adaptive_passes.py::test_device_entry_points_routed (own interpreter: torch first, then the
library; argument: the SIMD count).  Routed calls through the device entry points: a call on device slot 3 equals the
host-pointer call, its record is the model's, and a call on another slot afterwards sees no load left behind; a pool
of HBM-resident batches with completion counters, routed under no load and under a heavy one, gives every batch the
answers of a call of its own and every counter its batch's size."""
import sys

import numpy as np
import torch

torch.cuda.init()
sys.path.insert(0, ".")
import pick_ik_amd as pk  # noqa: E402
from oracle import oracle as O  # noqa: E402
from pick_ik_amd import robots  # noqa: E402
from pick_ik_amd.solver import Batch, STATS_DTYPE  # noqa: E402
from tests import route_model as M  # noqa: E402
from tests.test_gpu_adaptive_passes import LOAD_SLOT, SYNC_SLOT, problems  # noqa: E402

simds = int(sys.argv[1])
dev = torch.device("cuda", 0)
SLOT = 3
MARKS = "1,3,6,9"
KW = dict(memetic_population_size=24, memetic_max_generations=12, memetic_gd_max_iters=12)


def device_batch(goal, seed, off, D):
    B = len(goal)
    t = dict(goal=torch.from_numpy(goal).to(dev), seed=torch.from_numpy(seed).to(dev),
             sol=torch.empty(B, D, dtype=torch.float64, device=dev), st=torch.zeros(B, dtype=torch.int32, device=dev),
             c=torch.empty(B, dtype=torch.float64, device=dev), stats=torch.zeros(B, 3, dtype=torch.int64, device=dev),
             done=torch.zeros(1, dtype=torch.int32, device=dev))
    rec = Batch(B, t["goal"].data_ptr(), t["seed"].data_ptr(), None, off, t["sol"].data_ptr(), t["st"].data_ptr(),
                t["c"].data_ptr(), t["stats"].data_ptr(), t["done"].data_ptr())
    return t, rec


def results(t):
    return (t["sol"].cpu().numpy(), t["st"].cpu().numpy(), t["c"].cpu().numpy(),
            t["stats"].cpu().numpy().view(STATS_DTYPE).reshape(-1))


def same(a, b, what):
    for x, y, w in zip(a, b, ("solution", "status", "cost", "stats")):
        np.testing.assert_array_equal(x, y, err_msg=f"{what}: {w}")


def run(exact):
    ch = robots.panda()
    o = O.Oracle(ch)
    s = pk.Solver(ch, device=0, exact=exact)
    p = pk.default_params(**KW)
    model = M.Model(simds, 4, ch.dof, two_per_simd=2)
    s.set_option("two_per_simd", "2")
    s.set_option("passes", MARKS)
    rng = np.random.default_rng([0xDE, exact is None])
    st = torch.cuda.Stream(device=dev)
    # one call on a device slot, then a call on the synchronous slot: no load left behind
    goal, seed = problems(o, ch, rng, 110)
    host = s.solve_batch(p, goal, seed, rng_seed=9, problem_offset=40)
    t, _ = device_batch(goal, seed, 40, ch.dof)
    torch.cuda.synchronize()
    for load in (0, 10 * model.threshold):
        s.debug_regime(LOAD_SLOT, publish_load=load)
        with torch.cuda.stream(st):
            s.solve_batch_device(p, len(goal), t["goal"].data_ptr(), t["seed"].data_ptr(), t["sol"].data_ptr(),
                                 t["st"].data_ptr(), t["c"].data_ptr(), t["stats"].data_ptr(), rng_seed=9,
                                 problem_offset=40, stream=st.cuda_stream, slot=SLOT)
        torch.cuda.synchronize()
        rec = s.debug_regime(SLOT)
        s.debug_regime(LOAD_SLOT, publish_load=0)
        print(f"exact {exact} device slot {SLOT} load {load}: {rec}")
        assert rec is not None and len(rec) == 5
        model.check_record(rec, len(goal), load)
        assert all(n >= 1 for n, _, _ in rec), rec
        same(results(t), host, f"device slot {SLOT} load {load}")
        again = s.solve_batch(p, goal[:70], seed[:70], rng_seed=9, problem_offset=40)
        rec = s.debug_regime(SYNC_SLOT)
        print(f"exact {exact} after it: {rec}")
        assert rec is not None and all(other == 0 for _, other, _ in rec), rec
        same(again, [x[:70] for x in host], "a call behind the device call")
    # a pool of HBM-resident batches with completion counters
    sizes = [0, 1, 2, 37, 0, 64, 5, 1, 90, 0]
    goal, seed = problems(o, ch, rng, sum(sizes))
    perm = rng.permutation(len(goal))
    goal, seed = goal[perm], seed[perm]
    made, a = [], 0
    for k, n in enumerate(sizes):
        made.append(device_batch(goal[a:a + n].copy(), seed[a:a + n].copy(), 500 * k + 3, ch.dof) + (a, n, 500 * k + 3))
        a += n
    singles = [s.solve_batch(p, goal[a:a + n], seed[a:a + n], rng_seed=21, problem_offset=off) for _, _, a, n, off in made]
    torch.cuda.synchronize()
    for load in (0, 10 * model.threshold):
        for t, *_ in made:
            t["done"].zero_()
        torch.cuda.synchronize()
        s.debug_regime(LOAD_SLOT, publish_load=load)
        with torch.cuda.stream(st):
            s.solve_batches_device(p, [r for _, r, *_ in made], rng_seed=21, stream=st.cuda_stream, slot=SLOT)
        torch.cuda.synchronize()
        rec = s.debug_regime(SLOT)
        s.debug_regime(LOAD_SLOT, publish_load=0)
        print(f"exact {exact} device pool load {load}: {rec}")
        assert rec is not None and len(rec) == 5
        model.check_record(rec, sum(sizes), load)
        for k, ((t, _, a, n, off), single) in enumerate(zip(made, singles)):
            same(results(t), single, f"pool batch {k} load {load}")
            assert int(t["done"].item()) == n, (k, int(t["done"].item()), n)
    s.close()


for exact in (None, False):
    run(exact)
print("adaptive device check OK")
