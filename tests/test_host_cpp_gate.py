"""The approximate-solution gate through the C++ host mirror (pick_ik_amd/host/pick_ik_amd.hpp: Solver::gate,
Solver::set_approximate_gate): tests/native/gate_check.cpp compiles with plain g++ against the C ABI and, on a GPU,
returns what the C ABI returns."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "native", "gate_check.cpp")
EXE = os.path.join(ROOT, "tests", "native", "gate_check")


@pytest.fixture(scope="module")
def exe():
    import __graft_entry__ as g
    g.build()
    lib_dir = os.path.join(ROOT, "pick_ik_amd")
    if not os.path.exists(EXE) or os.path.getmtime(EXE) < max(
            os.path.getmtime(SRC), os.path.getmtime(os.path.join(lib_dir, "host", "pick_ik_amd.hpp"))):
        subprocess.run(["g++", "-std=c++17", "-O1", "-pthread", "-Wall", "-Wextra", "-Werror", SRC, "-o", EXE,
                        "-L" + lib_dir, "-lpick_ik_amd", "-Wl,-rpath," + lib_dir,
                        "-Wl,-rpath,/opt/rocm/lib"], check=True)
    return EXE


def test_cpp_gate_check_compiles(exe):
    assert os.path.exists(exe)


@pytest.mark.gpu
def test_cpp_host_mirror_gate(exe):
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "gate C++ checks OK" in r.stdout, r.stdout + r.stderr
