"""The routed launcher (CPU; needs only the build): its translation units carry the router kernel and NO copy of a
memetic kernel, the device source of the existing kernels is what it was, the parser of the option device_regime takes
"0" and "1" only, and the declarations are in place."""
import csv
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FLAVOURS = {"fast": "pik", "exact": "pik_exact", "common": "pik_common", "common_goals": "pik_common_goals"}


def test_route_objects_hold_the_router_kernel_and_no_memetic_kernel():
    import __graft_entry__ as g
    g.build()
    from pick_ik_amd import build as B
    from pick_ik_amd import kernel_resources as KR
    assert set(B.ROUTE_FLAVOURS) == set(FLAVOURS)
    for fl, ns in FLAVOURS.items():
        objs = B.family_objects("pik_route_inst.hip", fl)
        assert len(objs) == 16 and all(o[1] == "pik_route_inst.hip" for o in objs)
        for d, o in zip(B.DOFS, objs):
            if not os.path.exists(o[0] + ".res"):
                pytest.skip("no compiler remarks beside the objects (libraries built elsewhere)")
            kernels = [k for _, k, _ in KR.rows_of(open(o[0] + ".res").read(), fl)]
            assert kernels == [f"{ns}::route_kernel<{d}>"], (fl, d, kernels)
            # ... and the object refers to the memetic kernels without defining one
            syms = subprocess.run(["nm", "-C", o[0]], capture_output=True, text=True, check=True).stdout.splitlines()
            mem = [s for s in syms if "memetic_kernel<" in s]
            assert mem and all(re.match(r"^\s+U ", s) for s in mem), (fl, d, mem[:3])


def test_route_objects_are_compiled_with_their_flavour_s_flags():
    from pick_ik_amd import build as B
    for fl in FLAVOURS:
        inst = B.family_objects("pik_inst.hip", fl)
        assert inst == {"fast": B.library_objects(False)[2:18], "exact": B.library_objects(False)[18:34],
                        "common": B.library_objects(False)[34:50], "common_goals": B.library_objects(False)[50:66]}[fl]
        assert len(inst) == 16 and all(o[1] == "pik_inst.hip" for o in inst)
        for a, b in zip(inst, B.family_objects("pik_route_inst.hip", fl)):
            strip = lambda cmd: [x for x in cmd if not x.endswith((".o", ".hip"))]  # noqa: E731
            assert strip(B._cmd(*a, False)) == strip(B._cmd(*b, False)), (fl, a[0])
    assert "pik_route.hpp" not in {os.path.basename(f) for f in B._deps("pik_inst.hip", True)}
    assert "pik_kernels.hpp" not in {os.path.basename(f) for f in B._deps("pik_amd.hip", False)}


def test_committed_ledger_has_the_router_kernels():
    rows = {(r["flavour"], r["kernel"]): r for r in csv.DictReader(open(os.path.join(ROOT, "profiles", "r06_kernel_resources.csv")))}
    for fl, ns in FLAVOURS.items():
        for d in range(1, 17):
            r = rows[(fl, f"{ns}::route_kernel<{d}>")]
            assert int(r["scratch_bytes_per_lane"]) == 0 and int(r["vgpr_spills"]) == 0 and int(r["sgpr_spills"]) == 0
    assert len([k for k in rows if "route_kernel" in k[1]]) == 4 * 16


def test_existing_kernels_are_compiled_from_untouched_text():
    from pick_ik_amd import build as B
    from tests.test_path_cpu import PARENT_FLAVOUR_SHA
    assert {ns: B.flavour_sha(ns) for ns in B.FLAVOUR_FLAGS} == PARENT_FLAVOUR_SHA


def test_option_parser_accepts_0_and_1_only(tmp_path):
    from pick_ik_amd import build as B
    exe = str(tmp_path / "route_option_check")
    src = os.path.join(ROOT, "tests", "native", "route_option_check.cpp")
    r = subprocess.run([B.hipcc(), "-x", "hip", "--cuda-host-only", "-std=c++17", src, "-o", exe],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and "route option check OK" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]


def test_header_and_bindings_declare_the_debug_entry_point():
    header = open(os.path.join(ROOT, "include", "pick_ik_amd.h")).read()
    begin, end = header.index("[host-api-begin]"), header.index("[host-api-end]")
    assert begin < header.index("int32_t pikamd_debug_regime(") < end
    import __graft_entry__ as g
    g.build()
    import pick_ik_amd as pk
    from pick_ik_amd import solver
    assert "pikamd_debug_regime" in solver.EXPORTED_SYMBOLS
    assert solver.lib().pikamd_debug_regime.argtypes is not None
    assert callable(pk.Solver.debug_regime)
    assert ("PIK_DEVICE_REGIME", "device_regime") in pk.Solver.ENV_OPTIONS
