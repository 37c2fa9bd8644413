#!/usr/bin/env python3
"""What the validity step costs inside pikamd_cartesian_paths (pikamd_set_path_validity), and what a caller pays for
the same result without it.

Two sizes: the fixture "panda offsets" (P 70, W 12, cartesian_reference.OFFSETS) and P 4096 with W 16 (the same
generator).  The model is robots.panda_spheres() (its stock obstacles).  Three variants on ONE handle, alternated within
every repetition after a warm-up, medians of the repetitions, a host clock around synchronous host-pointer calls:

  off    the switch off: the call as it was before the step existed
  on     the switch on: the walk, then the cut and the relative test on the device
  host   what a caller writes today: the switch off with jump_factor 0, Solver.validity over all P * W rows, the cut,
         the blank rows, the fraction and the relative test in numpy (tests/pathvalid_reference.cut_cartesian's
         statements, vectorised where they can be)

`on` and `host` return the same arrays (checked here).  The numpy part of `host` is a loop over the paths; the time of
its two library calls alone is printed beside it -- a lower bound for any host implementation.  A record, not a gate.
usage: python tools/gpu/path_validity_latency.py [--reps 11] [--out profiles/path_validity_latency.txt]"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

import pick_ik_amd as pk  # noqa: E402
from pick_ik_amd import robots  # noqa: E402
from tests import cartesian_reference as CR  # noqa: E402
from tests import pathvalid_reference as PV  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=11)
ap.add_argument("--out", default=None)
args = ap.parse_args()

lines = []


def say(text):
    print(text, flush=True)
    lines.append(text)


chain = robots.panda()
s = pk.Solver(chain, device=0)
spheres, pairs = robots.panda_spheres()
s.set_validity_model(spheres, pairs)
p = pk.default_params(mode=1)
c = pk.Cartesian(**CR.OFFSETS)
c0 = pk.Cartesian(**dict(CR.OFFSETS, jump_factor=0.0))  # (OFFSETS names its min_steps: the poses are the same)


calls = []  # seconds host_variant spent in its two library calls, per run


def host_variant(start, target, W):
    t0 = time.perf_counter()
    plain0 = s.cartesian_paths(p, c0, start, target, W)
    P = len(start)
    valid = s.validity(plain0[0].reshape(P * W, -1))[0].reshape(P, W)
    calls.append(time.perf_counter() - t0)
    tested = np.arange(W)[None, :] < np.where(plain0[5] <= W, plain0[4], 0)[:, None]
    bad = ~valid & tested
    first = np.where(bad.any(axis=1), bad.argmax(axis=1), -1)
    return PV.cut_cartesian(plain0[:7], start, W, c.jump_factor, None, first)


say(f"path validity step: Panda, {len(spheres)} spheres, {len(pairs)} pairs, cartesian_paths with {CR.OFFSETS}; "
    f"{args.reps} alternated repetitions after 2 warm-up rounds, host clock around synchronous calls, milliseconds")
for name, P, W in (("panda offsets", 70, 12), ("P 4096", 4096, 16)):
    start, target = CR.offsets(chain, P=P)
    variants = {
        "off": lambda: (s.set_path_validity(False), s.cartesian_paths(p, c, start, target, W))[1],
        "on": lambda: (s.set_path_validity(True), s.cartesian_paths(p, c, start, target, W))[1],
        "host": lambda: (s.set_path_validity(False), host_variant(start, target, W))[1],
    }
    for _ in range(2):
        out = {k: f() for k, f in variants.items()}
    for x, y, w in zip(out["on"], out["host"], CR.NAMES):
        np.testing.assert_array_equal(x, y, err_msg=w)
    t = {k: [] for k in variants}
    del calls[:]
    for _ in range(args.reps):
        for k, f in variants.items():
            t0 = time.perf_counter()
            f()
            t[k].append(time.perf_counter() - t0)
    med = {k: float(np.median(v)) * 1e3 for k, v in t.items()}
    cut = int((out["on"][1] == PV.VALIDITY_REFUSED).any(axis=1).sum())
    say(f"  {name:14s} P = {P:5d} W = {W:2d}: off {med['off']:8.3f}   on {med['on']:8.3f} ({med['on'] - med['off']:+.3f})   "
        f"host alternative {med['host']:8.3f} (its two library calls alone {float(np.median(calls)) * 1e3:.3f}; the cut and the "
        f"relative test are a per-path numpy loop)   paths cut by the model {cut}, walked {int((out['on'][5] <= W).sum())}")
s.close()
if args.out:
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
