"""The validity model inside the path entry points through the C++ host mirror (pick_ik_amd/host/pick_ik_amd.hpp:
Solver::set_path_validity): tests/native/pathvalid_check.cpp compiles and links with plain g++ against the C ABI and,
on a GPU, cuts the paths where pikamd_validity_batch by hand cuts them."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "native", "pathvalid_check.cpp")
EXE = os.path.join(ROOT, "tests", "native", "pathvalid_check")


@pytest.fixture(scope="module")
def exe():
    import __graft_entry__ as g
    g.build()
    lib_dir = os.path.join(ROOT, "pick_ik_amd")
    if not os.path.exists(EXE) or os.path.getmtime(EXE) < max(
            os.path.getmtime(SRC), os.path.getmtime(os.path.join(lib_dir, "host", "pick_ik_amd.hpp")),
            os.path.getmtime(os.path.join(lib_dir, "libpick_ik_amd.so"))):
        subprocess.run(["g++", "-std=c++17", "-O1", "-pthread", "-Wall", "-Wextra", "-Werror", SRC, "-o", EXE,
                        "-L" + lib_dir, "-lpick_ik_amd", "-Wl,-rpath," + lib_dir,
                        "-Wl,-rpath,/opt/rocm/lib"], check=True)
    return EXE


def test_cpp_pathvalid_check_compiles_and_links(exe):
    assert os.path.exists(exe)


@pytest.mark.gpu
def test_cpp_host_mirror_path_validity(exe):
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "pathvalid C++ checks OK" in r.stdout, r.stdout + r.stderr
