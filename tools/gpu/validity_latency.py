#!/usr/bin/env python3
"""What the validity step costs inside the restart searches, and what pikamd_validity_batch costs on its own.

The fixture of tests/test_gpu_search_validity.py (the Panda of tests/search_reference.py, B = 64, rng_seed 1, the gated
parameters of tests/gate_reference.py: 8 local attempts, 4 memetic ones).  search_batch and search_global_batch are
timed on a handle without a model against a handle whose model has the shape of robots.panda_spheres() with every
radius 0: no pair of points overlaps, so the answers are the same arrays (checked here) and the difference is the step
alone -- the rows kernel in global mode, the call inside the search kernels in local mode.  Host clock around the
synchronous host-pointer calls; the two handles ALTERNATE within every repetition, medians over the repetitions, and
the spread of each side is printed beside the difference.  Then pikamd_validity_batch at n = 4096 (host pointers, and
the kernel alone by device events around the _device form).
usage: python tools/gpu/validity_latency.py [--reps 200] [--out profiles/validity_latency.txt]"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

import pick_ik_amd as pk  # noqa: E402
from pick_ik_amd import robots  # noqa: E402
from tests import gate_reference as GT  # noqa: E402
from tests import search_reference as SR  # noqa: E402
from tests.hip_buffers import DeviceBuffers  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=200)
ap.add_argument("--out", default=None)
args = ap.parse_args()

lines = []


def say(text):
    print(text, flush=True)
    lines.append(text)


def med_iqr(v):
    v = np.asarray(v) * 1e6
    return np.median(v), np.percentile(v, 75) - np.percentile(v, 25)


B = 64
chain = robots.panda()
plain = pk.Solver(chain, device=0)
model = pk.Solver(chain, device=0)
spheres, pairs = robots.panda_spheres()
model.set_validity_model([(a, c, 0.0) for a, c, _ in spheres], pairs)
for s in (plain, model):
    s.set_approximate_gate(GT.PANDA_GATE.cost_threshold, GT.PANDA_GATE.joint_threshold)
_, goals, seed, _ = SR.fixture("panda", lambda _: plain.fk, B)
say(f"validity step: Panda, B = {B}, {len(spheres)} spheres, {len(pairs)} pairs, radii 0 (identical answers); "
    f"{args.reps} alternated repetitions, host clock around the synchronous call, microseconds")
for family, K, kw, call in (("search_batch", GT.K, dict(GT.PANDA_KW), lambda s, p, K: s.search_batch(p, goals, seed, K, rng_seed=1)),
                            ("search_global_batch", GT.K_GLOBAL, dict(GT.PANDA_KW, **GT.GLOBAL_KW),
                             lambda s, p, K: s.search_global_batch(p, goals, seed, K, rng_seed=1))):
    p = pk.default_params(mode=1 if family == "search_batch" else 0, **kw)
    a, b = call(plain, p, K), call(model, p, K)  # (warm-up: the self test, the code objects)
    for x, y in zip(a, b):
        np.testing.assert_array_equal(x, y)
    t = {"plain": [], "model": []}
    for _ in range(args.reps):
        for name, s in (("plain", plain), ("model", model)):
            t0 = time.perf_counter()
            call(s, p, K)
            t[name].append(time.perf_counter() - t0)
    (mp, ip), (mm, im) = med_iqr(t["plain"]), med_iqr(t["model"])
    paired = np.median((np.asarray(t["model"]) - np.asarray(t["plain"])) * 1e6)
    say(f"  {family:20s} K = {K}: no model {mp:8.1f} (iqr {ip:5.1f})   zero-radius model {mm:8.1f} (iqr {im:5.1f})   "
        f"median of the paired differences {paired:+7.1f}   attempts run {int(a[4].sum())}")

n = 4096
rng = np.random.default_rng(0)
q = rng.uniform(chain.qmin, chain.qmax, size=(n, chain.dof))
full = pk.Solver(chain, device=0)
full.set_validity_model(spheres, pairs)
ok = full.validity(q)[0]
t = []
for _ in range(args.reps):
    t0 = time.perf_counter()
    full.validity(q)
    t.append(time.perf_counter() - t0)
m, i = med_iqr(t)
say(f"pikamd_validity_batch, n = {n} ({int(ok.sum())} valid): host pointers {m:.1f} us (iqr {i:.1f})")
d = DeviceBuffers()
hip = d.hip
import ctypes as C  # noqa: E402
ev = [C.c_void_p(), C.c_void_p()]
for e in ev:
    assert hip.hipEventCreate(C.byref(e)) == 0
dq, dv, dc = d.upload(q), d.alloc(4 * n), d.alloc(8 * n)
ms = []
for _ in range(args.reps + 5):
    assert hip.hipEventRecord(ev[0], None) == 0
    full.validity_device(n, dq, dv, dc)
    assert hip.hipEventRecord(ev[1], None) == 0
    assert hip.hipEventSynchronize(ev[1]) == 0
    out = C.c_float()
    assert hip.hipEventElapsedTime(C.byref(out), ev[0], ev[1]) == 0
    ms.append(out.value * 1e-3)
m, i = med_iqr(ms[5:])
say(f"pikamd_validity_batch_device, n = {n}: device events around the launch {m:.1f} us (iqr {i:.1f}); "
    f"{n / (m * 1e-6) / 1e6:.1f} M candidates/s")
d.free()
for s in (plain, model, full):
    s.close()
if args.out:
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
