"""What the path and search entry points refuse, in which order, with which text -- and which kernels every flavour of
handle reports for a parameter set -- held to a recording (tests/golden/abi_characterisation.json): callers match on
these texts, and bench.py keys its roofline inputs on the reported namespace.  No refusal runs a kernel; the names
cost one 64-problem solve per handle and global-mode parameter set.  The sizes the names are asked for (1, 16 and
2^20 units) lie far from the thresholds num_cu sets, so the recording does not depend on the exact CU count.

The four later families (pikamd_search_paths, pikamd_search_global_paths, pikamd_cartesian_paths and
pikamd_cartesian_waypoints) have a recording of their own, tests/golden/abi_characterisation_paths.json: refusals and
names, no solve.

Re-record (only when behaviour is MEANT to change): python -m tests.test_gpu_abi_characterisation <file> for the first
recording, python -m tests.test_gpu_abi_characterisation <file> paths for the second."""
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
GOLDEN_PATHS = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "abi_characterisation_paths.json")
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


# ---- the four later families: pikamd_search_paths, pikamd_search_global_paths, pikamd_cartesian_paths and
# pikamd_cartesian_waypoints (tests/golden/abi_characterisation_paths.json) ----
S = 2
PATH_FAMILIES = ("search_paths", "search_global_paths", "cartesian_paths", "cartesian_waypoints")
PATH_REQUIRED = {"search_paths": ("goal", "seed", "solution", "status"),
                 "search_global_paths": ("goal", "seed", "solution", "status"),
                 "cartesian_paths": ("start", "target", "solution", "status"),
                 "cartesian_waypoints": ("start", "targets", "solution", "status")}
PATH_ARRAY_NAMES = {"search_paths": A.STARTPATH_ARRAYS, "search_global_paths": A.STARTPATH_ARRAYS,
                    "cartesian_paths": A.CARTESIAN_ARRAYS, "cartesian_waypoints": A.WAYPOINT_ARRAYS}


def path_family_arrays(s, family):
    """every host array of one call of N paths, W rows (and S targets), the outputs filled with a pattern"""
    if family in ("search_paths", "search_global_paths"):
        return A.startpath_arrays(s, np.zeros((N, W, 7 * s.n_tips)), np.zeros((N, s.dof)), np.zeros((N, s.dof)), np.zeros(s.dof))
    inputs = dict(start=np.zeros((N, s.dof)), max_joint_step=np.zeros(s.dof))
    if family == "cartesian_paths":
        return dict(inputs, target=np.zeros((N, 7)), **A.cartesian_outputs(N, W, s.dof))
    return dict(inputs, targets=np.zeros((N, S, 7)), n_targets=np.full(N, S, dtype=np.int32),
                **A.waypoint_outputs(N, S, W, s.dof))


def path_refusals_of(s, s2, family, device):
    """[label, return code, pikamd_last_error()] of every refusal of one entry point of the four later families, in the
    order the code makes them.  s: a Panda handle; s2: a handle with several tip frames."""
    L = s._L
    cartesian, waypoints = family.startswith("cartesian"), family == "cartesian_waypoints"
    global_mode = family == "search_global_paths"
    good = pk.default_params(mode=0 if global_mode else 1)
    wrong_mode = pk.default_params(mode=1 if global_mode else 0)
    bad_params = pk.default_params(mode=0, memetic_elite_size=0) if global_mode else pk.default_params(mode=1, gd_step_size=0.0)
    motion = pk.Cartesian(frame=0, min_steps=0, max_translation=0.01, max_rotation=0.01, jump_factor=0.0)
    names = PATH_ARRAY_NAMES[family]
    handles, sets, frees = {"panda": s._h, "two tips": s2._h, None: None}, {}, []
    for who, x in (("panda", s), ("two tips", s2)):
        if device:  # real allocations: a call that (wrongly) passed every check would still be a valid one
            ptrs, free = A.device_buffers(len(names))
            frees.append(free)
            sets[who] = dict(zip(names, ptrs))
        else:
            sets[who] = path_family_arrays(x, family)
    pattern = {who: {k: v.copy() for k, v in a.items()} for who, a in sets.items() if not device}
    out = []

    def call(label, p=good, c=motion, n=N, w=W, k=K, n_seg=S, slot=0, handle="panda", **gone):
        a = {**sets[handle or "panda"], **gone}
        handle = handles[handle]
        if waypoints:
            rc = A.cartesian_waypoints(L, handle, p, c, n, n_seg, w, a, device=device, slot=slot)
        elif cartesian:
            rc = A.cartesian_paths(L, handle, p, c, n, w, a, device=device, slot=slot)
        else:
            rc = A.search_paths(L, handle, p, n, w, k, a, device=device, slot=slot, global_mode=global_mode)
        out.append([label, rc, A.last_error(L) if rc else ""])

    required = PATH_REQUIRED[family]
    try:
        call("solver NULL", handle=None)
        call("params NULL", p=None)
        call("wrong mode", p=wrong_mode)
        call("W = 0", w=0)
        call("P = -1", n=-1)
        s.set_option("joint_layout", "soa")
        call("joint_layout soa")
        call("joint_layout soa + bad params", p=bad_params)
        s.set_option("joint_layout", "aos")
        call("bad params", p=bad_params)
        if cartesian:
            call("pikamd_cartesian NULL", c=None)
            call("frame 3", c=pk.Cartesian(frame=3, min_steps=0, max_translation=0.01, max_rotation=0.01, jump_factor=0.0))
            call("min_steps -1", c=pk.Cartesian(frame=0, min_steps=-1, max_translation=0.01, max_rotation=0.01, jump_factor=0.0))
            call("neither step size positive", c=pk.Cartesian(frame=0, min_steps=0, max_translation=0.0, max_rotation=-1.0, jump_factor=0.0))
            call("several tip frames", handle="two tips")
            call("steps NULL, P = 3", steps=None)
            call("steps NULL, P = 0", n=0, steps=None)
        if waypoints:
            call("S = 0", n_seg=0)
            call("S > W", n_seg=W + 1)
        for r in required:
            call(f"{r} NULL", **{r: None})
        if not cartesian:
            call("max_attempts 0", k=0)
            call("max_attempts 65", k=65)
        if device:
            call("slot -1", slot=-1)
            call("slot MAX_SLOTS", slot=MAX_SLOTS)
        # the pairs that fix the order
        call("wrong mode + W = 0", p=wrong_mode, w=0)
        call("W = 0 + P = -1", w=0, n=-1)
        call("P = -1 + bad params", n=-1, p=bad_params)
        call("bad params + status NULL", p=bad_params, status=None)
        if cartesian:
            call("bad params + pikamd_cartesian NULL", p=bad_params, c=None)
            call("pikamd_cartesian NULL + steps NULL", c=None, steps=None)
            call("several tip frames + steps NULL", handle="two tips", steps=None)
            call("steps NULL + status NULL", steps=None, status=None)
        else:
            call("status NULL + max_attempts 0", status=None, k=0)
        if waypoints:
            call("steps NULL + S = 0", steps=None, n_seg=0)
            call("S > W + targets NULL", n_seg=W + 1, targets=None)
        if device:
            call(f"{required[0]} NULL + slot -1", slot=-1, **{required[0]: None})
            call("max_attempts 0 + slot -1" if not cartesian else "steps NULL + slot -1", slot=-1,
                 **(dict(steps=None) if cartesian else dict(k=0)))
            call("P = 0 + slot MAX_SLOTS", n=0, slot=MAX_SLOTS)
        # nothing to do: 0, and nothing is touched (the Cartesian pairs still need steps)
        call("n = 0", n=0)
        keep = ("steps",) if cartesian else ()
        call("n = 0, every array NULL", n=0, **{k: None for k in names if k not in keep})
        for who, arrays in pattern.items():
            for k, v in arrays.items():
                assert sets[who][k].tobytes() == v.tobytes(), (family, who, k)
    finally:
        s.set_option("joint_layout", "aos")
        for free in frees:
            free()
    return out


def collect_path_refusals():
    s, s2 = pk.Solver(robots.panda(), device=0), pk.Solver(robots.torso_dual_arm(), device=0)
    try:
        return {f"{family}{'_device' if device else ''}": path_refusals_of(s, s2, family, device)
                for family in PATH_FAMILIES for device in (False, True)}
    finally:
        s.close()
        s2.close()


def collect_path_names():
    """what the four name functions return, for every handle and parameter set: no solve, no kernel"""
    out = {}
    for hname, make in HANDLES.items():
        s = make()
        try:
            s.set_option("self_test", "off")  # (as collect_names: the names of an untested handle)
            for pname, kw in PARAMETER_SETS.items():
                p = pk.default_params(**kw)
                out[f"{hname}/{pname}"] = {
                    fn: {str(P): getattr(s, fn)(p, P) for P in (1, 1 << 20)}
                    for fn in ("search_paths_kernel_name", "search_global_paths_kernel_name", "cartesian_kernel_name",
                               "cartesian_waypoints_kernel_name")}
        finally:
            s.close()
    return out


@pytest.fixture(scope="module")
def golden():
    import __graft_entry__ as g
    g.build()
    return json.load(open(GOLDEN))


@pytest.fixture(scope="module")
def golden_paths():
    import __graft_entry__ as g
    g.build()
    return json.load(open(GOLDEN_PATHS))


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


def collect_paths():
    return {"refusals": collect_path_refusals(), "names": collect_path_names()}


def test_later_path_families_are_the_recorded_ones(golden_paths):
    """refusals and reported kernels of the four later families; runs no kernel beyond the handles' creation"""
    got = collect_paths()
    for part in ("refusals", "names"):
        assert sorted(got[part]) == sorted(golden_paths[part])
        for key, rec in got[part].items():
            assert rec == golden_paths[part][key], (part, key)


if __name__ == "__main__":
    # <file>: the recording of the three first families; <file> paths: that of the four later ones
    later = len(sys.argv) > 2 and sys.argv[2] == "paths"
    with open(sys.argv[1], "w") as f:
        json.dump(collect_paths() if later else {"refusals": collect_refusals(), "names": collect_names()}, f,
                  indent=1, sort_keys=True)
        f.write("\n")
