#!/usr/bin/env python3
"""What the routers decided in bench.py's default run (Panda, exact arithmetic, 8 calls of 64 batches of 4096 targets on
4 streams behind one warm-up call): the same inputs and the same enqueue order, but every timed call on a slot of its
own, so that the record of each of them (pikamd_debug_regime) can be read afterwards.  Prints, per timed call and
pass, the survivor count, the load the other slots had published and the variant the pass ran with -- with
--device-regime 0 (launch_solve serves the calls and leaves no record) the variant the host rule picks for the
survivor counts of a routed run of the same calls, under the regime the host chose for the call (three or more other
calls in flight when it was enqueued).  Writes the table as JSON to --out for tools/regime_trace.py --records.
usage: python tools/gpu/regime_report.py [--device-regime 0|1] [--threshold N] [--out records.json]"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
os.environ.setdefault("GPU_MAX_HW_QUEUES", "32")

import numpy as np  # noqa: E402
import torch  # noqa: E402

import pick_ik_amd as pk  # noqa: E402
from pick_ik_amd.solver import Batch  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--device-regime", type=int, default=1, choices=(0, 1))
ap.add_argument("--threshold", type=int, default=0)
ap.add_argument("--out", default=None)
args = ap.parse_args()

B, K, W, POOL, S, GS = 4096, 512, 64, 64, 4, 4
dev = torch.device("cuda", 0)
chain = pk.robots.panda()
D = chain.dof
solver = pk.Solver(chain, device=0, exact=True)
params = pk.default_params(memetic_population_size=128, memetic_elite_size=4, memetic_max_generations=100)
rng = np.random.default_rng(0x5049434B)
f64 = dict(dtype=torch.float64, device=dev)
seed_t = torch.from_numpy(np.tile(pk.robots.PANDA_HOME, (B, 1))).to(dev)
goals = []
for _ in range(K + W):
    q = torch.from_numpy(rng.uniform(chain.qmin, chain.qmax, size=(B, D))).to(dev)
    g = torch.empty(B, 7, **f64)
    solver.fk_device(B, q.data_ptr(), g.data_ptr(), torch.cuda.current_stream().cuda_stream)
    goals.append(g)
sols = [torch.empty(B, D, **f64) for _ in range(K + W)]
status = [torch.zeros(B, dtype=torch.int32, device=dev) for _ in range(K + W)]
costs = [torch.empty(B, **f64) for _ in range(K + W)]
stats = [torch.zeros(B, 3, dtype=torch.int64, device=dev) for _ in range(K + W)]
streams = [torch.cuda.Stream(device=dev) for _ in range(S)]
n_calls = K // POOL
torch.cuda.synchronize()


def run(first, count, slot0):
    for c, f in enumerate(range(first, first + count, POOL)):
        st = streams[c % S]
        recs = [Batch(B, goals[i].data_ptr(), seed_t.data_ptr(), None, i * B, sols[i].data_ptr(), status[i].data_ptr(),
                      costs[i].data_ptr(), stats[i].data_ptr(), None) for i in range(f, f + POOL)]
        with torch.cuda.stream(st):
            solver.solve_batches_device(params, recs, rng_seed=1234, stream=st.cuda_stream, slot=slot0 + c)


def timed(device_regime):
    solver.set_option("device_regime", str(device_regime))
    solver.set_option("regime_threshold", str(args.threshold) if args.threshold else "")
    run(0, W, 0)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    run(W, K, 0)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    ok = float(torch.stack(status[W:]).eq(pk.SUCCESS).sum().item())
    return ok / dt, [solver.debug_regime(c) for c in range(n_calls)]


for slot in range(n_calls):
    solver.reserve(params, B * POOL, slot=slot, stream=streams[slot % S].cuda_stream)
torch.cuda.synchronize()
value, records = timed(1)
if args.device_regime == 0:
    # the host rule: the survivor counts are the routed run's (they do not depend on the schedule), the regime of a
    # call is what the host saw when it enqueued it -- calls 0-2 latency, the others throughput
    from tests.test_gpu_device_regime import host_variant
    value, none = timed(0)
    assert all(r is None for r in none), none
    import glob
    for f in sorted(glob.glob("/sys/class/kfd/kfd/topology/nodes/*/properties"), key=lambda f: int(f.split("/")[-2])):
        try:
            props = dict(line.split()[:2] for line in open(f) if len(line.split()) >= 2)
        except OSError:
            continue
        if int(props.get("simd_count", 0)) > 0:
            simds = int(props["simd_count"])
            break
    records = [[(n, -1, host_variant(n, simds, c >= 3)) for n, _, _ in rec] for c, rec in enumerate(records)]
print(f"device_regime {args.device_regime}, threshold {args.threshold or 'default'}: {value:.0f} solves/s (this script's "
      f"own timing, every call on its own slot)")
print("per call and pass: survivors / others' load seen / variant (5 4 3 2 = 16 8 4 2 lanes per elite, 1 = one lane, "
      "7 = one lane two per SIMD; load -1: host rule, none published)")
for c, rec in enumerate(records):
    print(f"call {c}: " + "  ".join(f"{n}/{o}/{v}" for n, o, v in rec))
if args.out:
    json.dump({"device_regime": args.device_regime, "threshold": args.threshold, "value": value, "calls": records},
              open(args.out, "w"))
solver.close()
