"""pick_ik_amd/build.py: the rebuild rule.  An object is stale when the CODE of a file it includes changed -- comments
and blank space apart -- and the files a translation unit includes are found by following its #include lines
(pik_exact.hpp only for the exact flavours)."""
import os

from pick_ik_amd import build as B


def test_comments_and_blank_space_do_not_count_as_code():
    a = 'int a = 1; // one\n/* two */ const char* s = "x//y /*z*/"; char q = \'"\';   // "\nint b;'
    b = 'int a = 1;\nconst char* s = "x//y /*z*/";\n\n   char q = \'"\'; int b; /* trailing */'
    assert B._strip_comments(a) == B._strip_comments(b)
    assert B._strip_comments(a) != B._strip_comments(a.replace("int b", "long b"))
    assert '"x//y /*z*/"' in B._strip_comments(a)  # literals are not comments


def test_dependencies_follow_the_includes():
    base = lambda files: {os.path.basename(f) for f in files}
    fast = base(B._deps("pik_inst.hip", False))
    exact = base(B._deps("pik_inst.hip", True))
    assert {"pik_inst.hip", "pik_launch.hpp", "pik_kernels.hpp", "pik_math.hpp", "pik_host.hpp", "pick_ik_amd.h"} <= fast
    assert "pik_exact.hpp" not in fast and exact == fast | {"pik_exact.hpp"}
    abi = base(B._deps("pik_amd.hip", False))
    assert "pik_urdf.hpp" in abi and "pik_kernels.hpp" not in abi and "pik_host_solve.hpp" not in abi
    assert "pik_host_solve.hpp" in base(B._deps("pik_host_solve.hip", True))


def test_every_flavour_has_a_source_hash():
    # (hipcc -E of the device side: needs the compiler, no GPU)
    shas = {ns: B.flavour_sha(ns) for ns in B.FLAVOUR_FLAGS}
    assert all(len(v) == 16 for v in shas.values()) and len(set(shas.values())) == len(shas)


def test_the_headers_the_source_hash_leaves_out_hold_no_device_code():
    """flavour_sha is the hash of the DEVICE source: it skips the launcher headers, which must therefore define no
    kernel, device function, constant or LDS variable -- a kernel cannot hide from the hash in them"""
    assert B.HOST_LAUNCH_HEADERS == ("pik_launch.hpp", "pik_memetic_plan.hpp")
    inst = {os.path.basename(f) for f in B._deps("pik_inst.hip", True)}
    for name in B.HOST_LAUNCH_HEADERS:
        assert name in inst, name
        code = B._strip_comments(open(os.path.join(B.CSRC, name)).read())
        for word in ("__global__", "__device__", "__constant__", "__shared__"):
            assert word not in code, (name, word)


def test_memetic_plan_is_the_three_launchers_rules(tmp_path):
    """tests/native/memetic_plan_check.cpp: the plan as a host-only program, held to hand-computed schedules"""
    import subprocess
    exe = str(tmp_path / "memetic_plan_check")
    src = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "native", "memetic_plan_check.cpp")
    r = subprocess.run([B.hipcc(), "-x", "hip", "--cuda-host-only", "-std=c++17", src, "-o", exe],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and "memetic plan check OK" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]


#: the link list of the two libraries: blocks of (build directory, object stem), each one object per chain length
PRODUCT_BLOCKS = [("fast", "pik_inst"), ("exact", "pik_inst"), ("common", "pik_inst"), ("common_goals", "pik_inst"),
                  ("fast", "pik_path_inst"), ("exact", "pik_path_inst"),
                  ("fast", "pik_search_inst"), ("exact", "pik_search_inst"),
                  ("fast", "pik_route_inst"), ("exact", "pik_route_inst"), ("common", "pik_route_inst"),
                  ("common_goals", "pik_route_inst"),
                  ("fast", "pik_restart_inst"), ("exact", "pik_restart_inst"), ("common", "pik_restart_inst"),
                  ("common_goals", "pik_restart_inst")]
STRICT_BLOCKS = [("strict", "pik_inst"), ("strict", "pik_path_inst"), ("strict", "pik_search_inst"),
                 ("strict", "pik_restart_inst")]


def test_the_link_lists_are_these(monkeypatch):
    monkeypatch.delenv("PIK_ONLY_D", raising=False)
    monkeypatch.delenv("PIK_EXTRA_HIPCC_FLAGS", raising=False)
    for strict, blocks in ((False, PRODUCT_BLOCKS), (True, STRICT_BLOCKS)):
        home = "strict" if strict else "fast"
        want = [os.path.join(B.BUILD_DIR, home, "pik_amd.o"), os.path.join(B.BUILD_DIR, home, "pik_host_solve.o")]
        want += [os.path.join(B.BUILD_DIR, d, f"{stem}_d{n}.o") for d, stem in blocks for n in B.DOFS]
        objs = B.library_objects(strict)
        assert [o[0] for o in objs] == want
        assert [o[1] for o in objs[2:]] == [stem + ".hip" for _, stem in blocks for _ in B.DOFS]
        assert len(objs) == 2 + 16 * len(blocks)
    # every family is compiled with the flags of its flavour's pik_inst objects
    strip = lambda cmd: [x for x in cmd if not x.endswith((".o", ".hip"))]  # noqa: E731
    for family, (product, verification) in B.FAMILIES.items():
        for fl in product + verification:
            for a, b in zip(B.family_objects("pik_inst.hip", fl), B.family_objects(family, fl)):
                assert strip(B._cmd(*a, fl == "strict")) == strip(B._cmd(*b, fl == "strict")), (family, fl, b[0])
    # ... which are those flavour_sha hashes with the kernel text
    for fl, (ns, _) in B.FLAVOURS.items():
        cmd = B._cmd(*B.family_objects("pik_inst.hip", fl)[6], fl == "strict")
        flags = [x for x in cmd[cmd.index("-c") + 1:cmd.index("-o")]
                 if x != "-Rpass-analysis=kernel-resource-usage" and not x.startswith("-DPIK_INST_D=")]
        assert flags == B.FLAVOUR_FLAGS[ns], fl


def test_only_d_builds_the_other_lengths_as_stubs(monkeypatch):
    monkeypatch.setenv("PIK_ONLY_D", "6,7")
    for o in B.library_objects(False)[2:] + B.library_objects(True)[2:]:
        n = int(o[2][0].split("=")[1])
        assert o[2][0] == f"-DPIK_INST_D={n}" and (o[2][1:2] == ["-DPIK_INST_STUB=1"]) == (n not in (6, 7)), o


def test_the_sources_are_found_by_following_the_includes():
    names = {os.path.basename(f) for f in B._sources()}
    headers = {f for f in os.listdir(B.CSRC) if f.endswith(".hpp")}
    assert headers and headers <= names, headers - names
    assert {"pik_amd.hip", "pik_host_solve.hip", "pik_urdf.hpp", "pick_ik_amd.h", "build.py", *B.FAMILIES} <= names
    assert all(os.path.exists(f) for f in B._sources())


def test_a_call_cannot_qualify_for_the_common_and_the_literal_kernels():
    """pik_amd.hip flavour_of asks for the common flavours first and the literal kernels second; the order is
    immaterial as long as the step size up to which make_params_k sets line_delta (which the common flavours require)
    is not above the one from which a step needs the literal kernels.  Both constants, read from the sources."""
    import re
    host = B._strip_comments(open(os.path.join(B.CSRC, "pik_host.hpp")).read())
    abi = B._strip_comments(open(os.path.join(B.CSRC, "pik_amd.hip")).read())
    line_delta_up_to = re.search(r"k\.line_delta = \(p->gd_step_size <= ([0-9.e+-]+)\) \? 1 : 0;", host)
    literal_above = re.search(r"return needs_literal\(s\) \|\| \(p && p->gd_step_size > ([0-9.e+-]+)\);", abi)
    assert line_delta_up_to and literal_above
    assert float(line_delta_up_to.group(1)) == 1e-3 and float(literal_above.group(1)) == 1e-2
    assert float(line_delta_up_to.group(1)) <= float(literal_above.group(1))
    # ... and the common flavours do ask for line_delta, and exclude the chains that need the literal kernels
    eligible = abi[abi.index("bool common_eligible("):abi.index("Flavour flavour_of(")]
    assert "if (pk.line_delta == 0 ||" in eligible and "|| needs_literal(s)) return false;" in eligible
    # the parameter sets of the characterisation (tests/test_gpu_abi_characterisation.py): never both
    import numpy as np
    for step in (1e-4, 1e-3, float(np.nextafter(1e-3, 1.0)), 1e-2, 0.3):
        line_delta = step <= float(line_delta_up_to.group(1))
        literal_by_step = step > float(literal_above.group(1))
        assert not (line_delta and literal_by_step), step
