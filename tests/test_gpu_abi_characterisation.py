"""What the path and search entry points refuse, in which order, with which text -- and which kernels every flavour of
handle reports for a parameter set -- held to a recording (tests/golden/abi_characterisation.json): callers match on
these texts, and bench.py keys its roofline inputs on the reported namespace.  No refusal runs a kernel; the names
cost one 64-problem solve per handle and global-mode parameter set.  The sizes the names are asked for (1, 16 and
2^20 units) lie far from the thresholds num_cu sets, so the recording does not depend on the exact CU count.

Re-record (only when behaviour is MEANT to change): python -m tests.test_gpu_abi_characterisation <file>."""
import json
import os
import sys

import numpy as np
import pytest

import pick_ik_amd as pk
from pick_ik_amd import robots
from pick_ik_amd.solver import MAX_HOST_JOBS, MAX_SLOTS
from tests import abi_calls as A

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "abi_characterisation.json")
N, K, W = 3, 3, 3
REQUIRED = {"paths": ("goal", "start", "solution", "status"), "search": ("goal", "seed", "solution", "status")}


def refusals_of(s, family, device):
    """[label, return code, pikamd_last_error()] of every refusal of one entry point, in the order the code makes them"""
    L, h = s._L, s._h
    paths, global_mode = family == "paths", family == "search_global"
    good = pk.default_params(mode=0 if global_mode else 1)
    wrong_mode = pk.default_params(mode=1 if global_mode else 0)
    bad_params = pk.default_params(mode=0, memetic_elite_size=0) if global_mode else pk.default_params(mode=1, gd_step_size=0.0)
    names = A.PATH_ARRAYS if paths else A.SEARCH_ARRAYS
    if device:  # real allocations: a call that (wrongly) passed every check would still be a valid one
        ptrs, free = A.device_buffers(len(names))
        arrays = dict(zip(names, ptrs))
    else:
        free = lambda: None
        goals, seed = np.zeros((N, W, 7) if paths else (N, 7)), np.zeros((N, 7))
        arrays = A.path_arrays(s, goals, seed, np.zeros(7)) if paths else A.search_arrays(s, goals, seed, seed.copy(), K)
    pattern = {k: v.copy() for k, v in arrays.items() if not device}
    out = []

    def call(label, p=good, n=N, k=W if paths else K, slot=0, handle=h, **gone):
        a = {**arrays, **gone}
        if paths:
            rc = A.solve_paths(L, handle, p, n, k, a, device=device, slot=slot)
        else:
            rc = A.search(L, handle, p, n, k, a, device=device, slot=slot, global_mode=global_mode)
        out.append([label, rc, A.last_error(L) if rc else ""])

    try:
        call("solver NULL", handle=None)
        call("params NULL", p=None)
        call("wrong mode", p=wrong_mode)
        if paths:
            call("W = 0", k=0)
            call("P = -1", n=-1)
        else:
            call("max_attempts 0", k=0)
            call("max_attempts 65", k=65)
            call("B = -1", n=-1)
        s.set_option("joint_layout", "soa")
        call("joint_layout soa")
        call("joint_layout soa + bad params", p=bad_params)
        s.set_option("joint_layout", "aos")
        call("bad params", p=bad_params)
        for r in REQUIRED["paths" if paths else "search"]:
            call(f"{r} NULL", **{r: None})
        if device:
            call("slot -1", slot=-1)
            call("slot MAX_SLOTS", slot=MAX_SLOTS)
            call("goal NULL + slot -1", slot=-1, goal=None)
            call("bad params + slot MAX_SLOTS", p=bad_params, slot=MAX_SLOTS)
        call("wrong mode + count 0", p=wrong_mode, k=0)
        call("count 0 + n = -1", k=0, n=-1)
        call("n = -1 + bad params", n=-1, p=bad_params)
        call("bad params + status NULL", p=bad_params, status=None)
        # nothing to do: 0, and nothing is touched
        call("n = 0", n=0)
        call("n = 0, every array NULL", n=0, **{k: None for k in names})
        for k, v in pattern.items():
            assert arrays[k].tobytes() == v.tobytes(), (family, k)
    finally:
        s.set_option("joint_layout", "aos")
        free()
    return out


def collect_refusals():
    s = pk.Solver(robots.panda(), device=0)
    try:
        return {f"{family}{'_device' if device else ''}": refusals_of(s, family, device)
                for family in ("paths", "search", "search_global") for device in (False, True)}
    finally:
        s.close()


def mimic_panda():
    from tests.test_mimic_cpu import CASES, with_mimic
    name, k, master, mult, off = CASES[0]
    return with_mimic(np.random.default_rng(5 + k), robots.by_name(name), k, master, mult, off)[0]


HANDLES = {
    "panda_fast": lambda: pk.Solver(robots.panda(), device=0, exact=False),
    "panda_exact": lambda: pk.Solver(robots.panda(), device=0, exact=True),
    "floating": lambda: pk.Solver(robots.floating_panda(), device=0, exact=False),
    "mimic": lambda: pk.Solver(mimic_panda(), device=0, exact=False),
    "dual_arm": lambda: pk.Solver(robots.torso_dual_arm(), device=0, exact=False),
    "panda_strict": lambda: pk.Solver(robots.panda(), device=0, strict=True),
}
STEPS = {"step_1e-3": 1e-3, "step_above_1e-3": float(np.nextafter(1e-3, 1.0)), "step_1e-2": 1e-2, "step_0.3": 0.3}
PARAMETER_SETS = {
    "default": {},
    "mode_1": dict(mode=1),
    "joint_goal": dict(center_joints_weight=0.1),
    "elites_2": dict(memetic_elite_size=2),
    "species_2": dict(memetic_num_threads=2),
    **{k: dict(gd_step_size=v) for k, v in STEPS.items()},
    **{k + "_mode_1": dict(mode=1, gd_step_size=v) for k, v in STEPS.items()},
}


def collect_names():
    out = {}
    rng = np.random.default_rng(3)
    for hname, make in HANDLES.items():
        s = make()
        try:
            s.set_option("self_test", "off")  # (it may switch widths off: the names are those of an untested handle)
            ch = s.chain
            lo = np.where(np.isfinite(ch.qmin), ch.qmin, -0.5)
            q = rng.uniform(lo, np.where(np.isfinite(ch.qmax), ch.qmax, 0.5), size=(64, ch.dof))
            if hname == "floating":
                q[:, :7] = robots.FLOATING_PANDA_HOME[:7]
            goals, seed = s.fk(q), np.tile(q[:1], (64, 1))
            for pname, kw in PARAMETER_SETS.items():
                p = pk.default_params(**kw)
                rec = {"kernel_name": s.kernel_name(p),
                       "path_kernel_name": {str(P): s.path_kernel_name(p, P) for P in (1, 1 << 20)},
                       "search_kernel_name": {f"{B},{k}": list(s.search_kernel_name(p, B, k))
                                              for B, k in ((1, 1), (1, 16), (1 << 20, 16))}}
                if p.mode == 0:
                    s.solve_batch(p, goals, seed, rng_seed=5)
                    rec["routed"] = s.debug_regime(MAX_SLOTS + MAX_HOST_JOBS - 1) is not None
                out[f"{hname}/{pname}"] = rec
        finally:
            s.close()
    return out


@pytest.fixture(scope="module")
def golden():
    import __graft_entry__ as g
    g.build()
    return json.load(open(GOLDEN))


def test_refusals_are_the_recorded_ones(golden):
    got = collect_refusals()
    assert sorted(got) == sorted(golden["refusals"])
    for entry, rows in got.items():
        assert rows == golden["refusals"][entry], entry


def test_reported_kernels_are_the_recorded_ones(golden):
    got = collect_names()
    assert sorted(got) == sorted(golden["names"])
    for key, rec in got.items():
        assert rec == golden["names"][key], key


if __name__ == "__main__":
    with open(sys.argv[1], "w") as f:
        json.dump({"refusals": collect_refusals(), "names": collect_names()}, f, indent=1, sort_keys=True)
        f.write("\n")
