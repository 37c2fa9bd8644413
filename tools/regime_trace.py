#!/usr/bin/env python3
"""Which kernel variant served every pass of every call, and how the run ends, from a rocprofv3 kernel-trace csv of
`python bench.py --gpus 1` (the default run: 8 timed calls of 64 batches on 4 streams behind one warm-up call).

The host enqueues a call's kernels in one go, so in dispatch order a call is its pass-0 kernel followed by one group
of candidate variants per compaction pass, each group ending with the two-per-SIMD one-lane kernel
(memetic_kernel<D,1,false,2>).  WHICH variant of a group served the pass cannot be read off the durations: the
candidates that return at once still wait for a place on a chip that other pools' persistent wavefronts fill, and that
wait is inside their duration.  It comes from --records, the table tools/gpu/regime_report.py writes for the same
calls (the routers' own record with device_regime = 1, the host rule applied to the same survivor counts with 0);
without --records the longest kernel of a group is taken.  A duration is therefore "queued behind other pools +
running".  Router kernels (route_kernel, device_regime = 1) are counted but take no part in the grouping.
Reported: per timed call the variant and duration of every pass; the end phase -- from the end of the last kernel of
a chip-filling pass (served by <D,1,false,2>) to the end of the last kernel -- with the kernels that ran in it and the
time-weighted sum of their grids (wavefronts launched: an upper bound of the resident ones, a persistent grid is sized
by the call, not by the survivors); the time the first three timed calls spent in wide variants (more than one lane per
elite) while another call's kernel was running.
usage: tools/regime_trace.py <kernel_trace.csv> [--records records.json] [--passes 11] [--calls 8] [--min-us 30]"""
import csv
import json
import re
import sys

a = sys.argv[1:]
opt = lambda k, d: type(d)(a[a.index(k) + 1]) if k in a else d  # noqa: E731
n_pass, n_calls, min_us = opt("--passes", 11), opt("--calls", 8), opt("--min-us", 30.0)
rows = list(csv.DictReader(open(a[0])))
key = "Dispatch_Id" if "Dispatch_Id" in rows[0] else "Start_Timestamp"
rows.sort(key=lambda r: int(r[key]))
routers = sum("route_kernel" in r["Kernel_Name"] for r in rows)
K = []
for r in rows:
    m = re.search(r"memetic_kernel<([^>]*)>", r["Kernel_Name"])
    if m:
        t = [x.strip() for x in m.group(1).split(",")]
        lanes = int(t[1])
        occ = int(t[3]) if len(t) > 3 else 1
        K.append(dict(v=f"{lanes}" + ("x2" if occ == 2 else ""), lanes=lanes, occ=occ, s=int(r["Start_Timestamp"]),
                      e=int(r["End_Timestamp"]), waves=int(r.get("Grid_Size_X", r.get("Grid_Size", 0)) or 0) // 64))
for k in K:
    k["us"] = (k["e"] - k["s"]) / 1e3
big = max(k["waves"] for k in K) // 2
start = next(i for i, k in enumerate(K) if k["waves"] >= big)  # (in front of it: the self test's small calls)
calls, i = [], start
while i < len(K):
    call, seen = [[K[i]]], 0
    i += 1
    group = []
    while i < len(K) and seen < n_pass:
        group.append(K[i])
        if K[i]["occ"] == 2:
            call.append(group)
            group, seen = [], seen + 1
        i += 1
    if seen == n_pass:
        calls.append(call)
calls = calls[-n_calls:]
for c, call in enumerate(calls):
    for g in call:
        for k in g:
            k["call"] = c
records = json.load(open(opt("--records", ""))) if "--records" in a else None
ID = {5: (16, 1), 4: (8, 1), 3: (4, 1), 2: (2, 1), 1: (1, 1), 7: (1, 2)}
work = []
for c, call in enumerate(calls):
    w = []
    for p, g in enumerate(call):
        pick = max(g, key=lambda k: k["us"])
        if records:
            n, load, vid = records["calls"][c][p]
            hit = [k for k in g if (k["lanes"], k["occ"]) == ID.get(vid)]
            pick = hit[0] if hit else pick
            pick["n"], pick["load"] = n, load
        w.append(pick)
    work.append(w)
t0 = min(k["s"] for k in work[0])
t_end = max(k["e"] for call in calls for g in call for k in g)
region = (t_end - t0) / 1e6
print(f"{len(calls)} timed calls, {n_pass + 1} passes each; {routers} router dispatches in the trace; timed region "
      f"(first kernel of the first timed call -> last kernel end) {region:.2f} ms")
print("pass:      " + " ".join(f"{p:>9d}" for p in range(n_pass + 1)))
for c, w in enumerate(work):
    print(f"call {c} var " + " ".join(f"{(k['v'] if k['us'] >= min_us else '-'):>9s}" for k in w))
    if records:
        print(f"       n   " + " ".join(f"{k['n']:9d}" for k in w))
        if records["device_regime"]:
            print(f"     load  " + " ".join(f"{k['load']:9d}" for k in w))
    print(f"       ms  " + " ".join(f"{k['us'] / 1e3:9.3f}" for k in w) +
          f"   start +{(w[0]['s'] - t0) / 1e6:7.2f} end +{(max(k['e'] for k in w) - t0) / 1e6:7.2f} ms")
allw = [k for w in work for k in w if k["us"] >= min_us]
bulk_end = max(k["e"] for k in allw if k["occ"] == 2)
tail = sorted((k for k in allw if k["e"] > bulk_end), key=lambda k: k["s"])
end_ms = (t_end - bulk_end) / 1e6
wave_ns = sum((k["e"] - max(k["s"], bulk_end)) * k["waves"] for k in tail)
print(f"end phase (last chip-filling kernel's end -> last kernel's end): {end_ms:.2f} ms = {100 * end_ms / region:.1f} % "
      f"of the timed region; wavefronts launched by the kernels in it, time-weighted: {wave_ns / max(1, t_end - bulk_end):.0f}")
for k in tail:
    print(f"   call {k['call']} <{k['v']:>4s}> +{(max(k['s'], bulk_end) - bulk_end) / 1e6:7.2f} ms  {k['us'] / 1e3:7.3f} ms  grid {k['waves']} waves")
wide = 0.0
for k in allw:
    if k["call"] < 3 and k["lanes"] > 1 and any(o["call"] != k["call"] and o["s"] < k["e"] and o["e"] > k["s"] for o in allw):
        wide += k["us"]
print(f"wide variants (> 1 lane per elite) of calls 0-2 while another call's kernel ran: {wide / 1e3:.2f} ms = "
      f"{100 * wide / 1e3 / region:.1f} % of the timed region")
