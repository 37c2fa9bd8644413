#!/usr/bin/env python3
"""Latency of pikamd_solve_paths against the host loop of solve_batch calls it replaces (tests/path_reference.py
host_loop): Panda, joint-space-line waypoints, W = 32, the default (exact) handle; P = 1 and P = 4096.  Both sides
warmed, alternated 21 times, medians of a host clock around calls that end synchronised.

usage: python tools/path_latency.py [out.txt]     the figures (profiles/path_latency.txt is a run of this)
       python tools/path_latency.py --kernel-only  a few solve_paths calls and nothing else: the program to put behind
                                                   `rocprofv3 --kernel-trace --stats --` for the kernel's own row
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import pick_ik_amd as pk  # noqa: E402
from pick_ik_amd import robots  # noqa: E402
from tests import path_reference as PR  # noqa: E402

W = 32


def main():
    ch = robots.panda()
    s = pk.Solver(ch, device=0)
    p = pk.default_params(mode=1)
    if "--kernel-only" in sys.argv:
        for P in (1, 4096):
            goals, start = PR.joint_lines(ch, s.fk, P=P, W=W)
            for _ in range(5):
                s.solve_paths(p, goals, start)
        return
    lines = ["pikamd_solve_paths against the loop of W local-mode pikamd_solve_batch calls (Panda, joint-space lines, "
             f"W = {W}, default exact handle; medians of 21 alternated repetitions, host clock, synchronised calls)"]
    for P in (1, 4096):
        goals, start = PR.joint_lines(ch, s.fk, P=P, W=W)
        reached = s.solve_paths(p, goals, start)[4]
        paths, loop, tp, tl = PR.time_paths_against_loop(s, p, goals, start, reps=21)
        lines.append(f"P = {P:5d}  {s.path_kernel_name(p, P):44s} complete paths {int((reached == W).sum())}/{P}  "
                     f"solve_paths {paths * 1e3:9.3f} ms (min {min(tp) * 1e3:.3f}, max {max(tp) * 1e3:.3f})  "
                     f"loop {loop * 1e3:9.3f} ms (min {min(tl) * 1e3:.3f}, max {max(tl) * 1e3:.3f})  "
                     f"loop / solve_paths {loop / paths:.2f}")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    out = [a for a in sys.argv[1:] if not a.startswith("--")]
    if out:
        with open(out[0], "w") as f:
            f.write(text)
    s.close()


if __name__ == "__main__":
    main()
