"""The validity model inside the path entry points (CPU): the normative loop with the step `refused`
(tests/pathvalid_reference.py) over the CPU oracle on the fixtures of the GPU tests -- each must reach every class, so
that the GPU comparison (tests/test_gpu_pathvalid.py) cannot pass on one branch only --, the two forms of the reference
(stop at the refused answer; walk, then cut) against one another, the shape of the rows behind a validity stop, the
declarations, the build tables, the resource ledger and the refusals that need no device."""
import csv
import ctypes as C
import hashlib
import os
import re

import numpy as np
import pytest

from tests import cartesian_reference as CR
from tests import path_reference as PR
from tests import pathvalid_reference as PV
from tests import polyline_reference as LR
from tests.test_path_cpu import PARENT_FLAVOUR_SHA

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOL = "pikamd_set_path_validity"
FAMILY = "pik_pathvalid_inst.hip"
KERNELS = ("pathvalid_paths_kernel", "pathvalid_motion_kernel", "pathvalid_segment_kernel")
#: sha256 of profiles/r06_kernel_resources.csv as committed BEFORE this family; the committed ledger without the
#: family's rows must still be that text
PARENT_LEDGER_SHA256 = "af752b9bdc4c787449910be778ba2b3f4c83cd1f59ca750b7af4a094710f5c4f"


@pytest.fixture(params=["portable", "fma"])
def mode(request):
    return request.param


@pytest.fixture(scope="module")
def pk():
    import __graft_entry__ as g
    g.build()
    import pick_ik_amd
    return pick_ik_amd


def _same(a, b, names, what):
    for x, y, w in zip(a, b, names):
        np.testing.assert_array_equal(x, y, err_msg=f"{what}: {w}")


# ---- the fixtures reach every class -------------------------------------------------------------------
def test_placed_obstacles_reach_every_class(oracle_mod, mode):
    fx = PV.placed_paths(oracle_mod, mode)
    spheres, pairs = fx["model"]
    assert len(fx["chosen"]) == PV.N_OBSTACLES and len(spheres) == 21 and len(pairs) == 123
    got = PV.cut_classes(fx["plain"][1], fx["plain"][4], fx["want"][1], fx["want"][4], PV.W_PATHS)
    print(f"placed obstacles [{mode}]: left alone / cut at row 0 / cut inside / distinct inside rows / cut on a "
          f"solver-stopped path = {got}")
    assert all(g >= m for g, m in zip(got, PV.MINIMA_PATHS)), (got, PV.MINIMA_PATHS)
    # the chosen paths are cut, at their obstacle's row or in front of it (an obstacle of another path)
    at = np.argmax(fx["want"][1] == PV.VALIDITY_REFUSED, axis=1)
    for p, k in zip(fx["chosen"], fx["rows"]):
        assert fx["want"][1][p, at[p]] == PV.VALIDITY_REFUSED and at[p] <= k, (p, k, at[p])


@pytest.mark.parametrize("limit", [None, 0.1])
def test_offsets_fixture_reaches_every_class(oracle_mod, pk, mode, limit):
    fx = PV.placed_offsets(oracle_mod, pk, mode, limit)
    cl = PV.cartesian_classes(fx["plain"][1], fx["held_plain"], np.where(fx["steps"] <= PV.W_OFFSETS, fx["steps"], -1),
                              fx["want"][1], fx["held"])
    print(f"placed offsets [{mode}] limit {limit}: {cl}, obstacles on {fx['chosen']} at {fx['rows']}")
    if limit is None:  # the fixture as the table has it; with a step limit few paths are complete: they are compared all the same
        for k, m in PV.MINIMA_CARTESIAN.items():
            assert cl[k] >= m, (k, cl)
    else:
        assert cl["alone"] >= 4 and cl["inside"] >= 1 and cl["at0"] >= 1 and cl["moved"] >= 1, cl
    assert (fx["steps"] > PV.W_OFFSETS).sum() >= 1  # (a path that is not walked: left alone by the step)


@pytest.mark.parametrize("limit", [None, 0.1])
def test_polylines_fixture_reaches_every_class(oracle_mod, pk, mode, limit):
    fx = PV.placed_polylines(oracle_mod, pk, mode, limit)
    ip, held = fx["info_plain"], fx["info"]["held"]
    cl = PV.cartesian_classes(fx["plain"][1], ip["held"], np.where(ip["kind"] == LR.COMPLETE, ip["held"], -1),
                              fx["want"][1], held)
    later = PV.cut_behind_the_first_segment(ip["held"], held, fx["want"][8], fx["info"]["seg"])
    print(f"placed polylines [{mode}] limit {limit}: {cl}, cut in a segment behind the first: {later}")
    for k, m in PV.MINIMA_CARTESIAN.items():
        assert cl[k] >= m, (k, cl)
    assert later >= 2, later


# ---- the two forms of the reference ---------------------------------------------------------------------
def test_stopping_at_the_refusal_is_walking_and_cutting(oracle_mod, pk, mode):
    O = oracle_mod
    from tests import validity_reference as V
    fx = PV.placed_paths(O, mode)
    with O.math_mode(mode):
        valid_fn = V.valid_of(V.oracle_fk_of(O, fx["chain"]), fx["model"])
        _same(PV.cut_paths(fx["plain"], fx["start"], valid_fn), fx["want"], CR.NAMES, f"paths [{mode}]")
        for limit in (None, 0.1):
            fo = PV.placed_offsets(O, pk, mode, limit)
            valid_fn = V.valid_of(V.oracle_fk_of(O, fo["chain"]), fo["model"])
            got = PV.cut_cartesian(fo["plain0"], fo["start"], PV.W_OFFSETS, CR.OFFSETS["jump_factor"], valid_fn)
            _same(got, fo["want"], CR.NAMES, f"offsets [{mode}] limit {limit}")


def test_a_jumped_answer_is_not_tested():
    """one path, two waypoints: the second answer jumps AND is invalid -- PATH_JUMP, not VALIDITY_REFUSED"""
    sols = iter([np.array([[0.1, 0.0]]), np.array([[0.9, 0.0]])])
    solve = lambda g, sd: (next(sols), np.array([1], dtype=np.int32), np.array([0.25]), np.zeros(1, dtype=PR.STATS_DTYPE))
    valid_fn = lambda q: q[:, 0] < 0.5
    out = PV.reference_paths(solve, np.zeros((1, 2, 7)), np.zeros((1, 2)), np.array([0.5, 0.5]), valid_fn)
    assert out[1].tolist() == [[1, PR.PATH_JUMP]] and out[4].tolist() == [1]


# ---- the rows behind a validity stop ----------------------------------------------------------------------
def test_row_shape_behind_a_validity_stop(oracle_mod, pk, mode):
    fx = PV.placed_paths(oracle_mod, mode)
    sol, st, cost, stats, reached = fx["want"]
    psol, pst, pcost, pstats, preached = fx["plain"]
    seen = 0
    for p in range(PV.P_PATHS):
        hit = np.nonzero(st[p] == PV.VALIDITY_REFUSED)[0]
        if len(hit) == 0:
            continue
        assert len(hit) == 1
        f = int(hit[0])
        seen += 1
        held = fx["start"][p] if f == 0 else sol[p, f - 1]
        assert reached[p] == f and (st[p, :f] > 0).all()
        np.testing.assert_array_equal(sol[p, :f], psol[p, :f])  # (in front of the cut: the plain walk)
        np.testing.assert_array_equal(sol[p, f:], np.tile(held, (PV.W_PATHS - f, 1)))
        # the refused row keeps the cost and the counters of its solve
        assert cost[p, f] == pcost[p, f] and stats[p, f] == pstats[p, f] and stats["cost_evals"][p, f] > 0
        assert (st[p, f + 1:] == PR.NOT_ATTEMPTED).all() and (cost[p, f + 1:] == 0.0).all()
        assert (stats[p, f + 1:] == PV.ZERO_STATS).all()
    assert seen >= 12
    # the two-factor fraction: r / n of the cut, times (i + 1) / (r + 1) of a relative stop behind it
    fo = PV.placed_offsets(oracle_mod, pk, mode)
    sol, st, cost, stats, reached, steps, fraction = fo["want"]
    both = 0
    for p in range(len(steps)):
        if steps[p] > PV.W_OFFSETS:
            assert fraction[p] == 0.0 and reached[p] == 0 and (st[p] == 0).all()
            continue
        r = int(fo["held"][p])
        want = np.float64(r) / np.float64(steps[p])
        if reached[p] != r:
            assert st[p, reached[p]] == CR.PATH_RELATIVE_JUMP
            want = want * (np.float64(reached[p] + 1) / np.float64(r + 1))
            both += r < steps[p] and (fo["want"][0][p, r:] == fo["want"][0][p, r]).all()
        elif r < steps[p]:
            assert st[p, r] < 0
        assert fraction[p] == want, p
    assert both >= 1


# ---- declarations ---------------------------------------------------------------------------------------
def test_header_declares_the_switch_inside_the_host_api_block():
    text = open(os.path.join(ROOT, "include", "pick_ik_amd.h")).read()
    block = text[text.index("[host-api-begin]"):text.index("[host-api-end]")]
    assert "int32_t pikamd_set_path_validity(pikamd_solver* s, int32_t on);" in block
    assert re.search(r"refused = applies and st > 0 and not jump and valid\(sol\) == 0", block)
    assert "refused ? PIKAMD_VALIDITY_REFUSED" in block
    assert "pikamd_search_paths* and pikamd_search_global_paths* keep ignoring the model" in block
    # nothing was taken away: the sentences earlier tests look for are still there
    assert "IGNORE it" in text and "a validity" in text
    assert text.count("#define PIKAMD_VALIDITY_REFUSED") == 1 and "-1005" not in text


def test_both_libraries_export_the_symbol_and_the_mirrors_exist(pk):
    from pick_ik_amd import solver
    assert SYMBOL in solver.EXPORTED_SYMBOLS
    for strict in (False, True):
        assert hasattr(solver.lib(strict), SYMBOL)
    assert callable(pk.Solver.set_path_validity)
    hpp = open(os.path.join(ROOT, "pick_ik_amd", "host", "pick_ik_amd.hpp")).read()
    assert re.search(r"void set_path_validity\(bool on\) const", hpp) and "pikamd_set_path_validity(h_" in hpp
    shim = open(os.path.join(ROOT, "pick_ik_amd", "host", "pick_ik_plugin_shim.cpp")).read()
    assert "path_validity" not in shim  # (KinematicsBase has no Cartesian path)


def test_refusals_without_a_device(pk):
    from pick_ik_amd import solver
    for strict in (False, True):
        L = solver.lib(strict)
        L.pikamd_set_path_validity.argtypes = [C.c_void_p, C.c_int32]
        L.pikamd_last_error.restype = C.c_char_p
        assert L.pikamd_set_path_validity(None, 1) == -1 and b"NULL" in L.pikamd_last_error()
        assert L.pikamd_set_path_validity(None, 2) == -1 and b"expected 0 or 1" in L.pikamd_last_error()


# ---- the build tables and the ledger ------------------------------------------------------------------------
def test_build_tables_name_the_family():
    from pick_ik_amd import build as Bd
    assert Bd.FAMILIES[FAMILY] == (("exact",), ("strict",))
    order = Bd.APPENDED_FAMILIES
    assert order.index(FAMILY) < order.index("pik_globalpath_inst.hip") and order[-1] == "pik_globalpath_inst.hip"
    for strict, flavours, gp in ((False, ("exact",), ("fast", "exact")), (True, ("strict",), ("strict",))):
        linked = Bd.link_objects(strict)
        objs = [o for o in linked if "pik_pathvalid" in o[0]]
        assert objs == [o for fl in flavours for o in Bd.family_objects(FAMILY, fl)] and len(objs) == 16
        last = [o for fl in gp for o in Bd.family_objects("pik_globalpath_inst.hip", fl)]
        assert linked[-len(last):] == last and linked.index(objs[-1]) < linked.index(last[0])
        assert not any("pik_pathvalid" in o[0] for o in Bd.library_objects(strict))
    assert "+pathvalid" in open(Bd.__file__).read()


def test_the_kernels_are_reached_from_no_existing_translation_unit():
    from pick_ik_amd import build as Bd
    for tu in Bd.FAMILIES:
        if tu != FAMILY:
            for f in Bd._deps(tu, True):
                assert "pik_pathvalid" not in os.path.basename(f), (tu, f)
    ops = Bd._strip_comments(open(os.path.join(Bd.CSRC, "pik_pathvalid_ops.hpp")).read())
    assert not re.search(r"__global__|__device__|__shared__|__constant__", ops)
    seen = [os.path.basename(f) for f in Bd._deps("pik_amd.hip", True)]
    assert "pik_pathvalid_ops.hpp" in seen and "pik_pathvalid.hpp" not in seen
    seen = [os.path.basename(f) for f in Bd._deps(FAMILY, True)]
    assert "pik_validity.hpp" in seen and "pik_polyline.hpp" in seen and "pik_cartesian.hpp" in seen
    # the relative test is cartesian_tail's own statements: called, not restated
    text = Bd._strip_comments(open(os.path.join(Bd.CSRC, "pik_pathvalid.hpp")).read())
    assert "cartesian_tail<D>(" in text and "PIKAMD_PATH_RELATIVE_JUMP_K" not in text and "validity_clear<D>(" in text


def _ledger(path):
    return {(r["flavour"], r["kernel"]): r for r in csv.DictReader(open(path))}


def test_committed_ledger_gained_the_kernels_and_lost_nothing():
    path = os.path.join(ROOT, "profiles", "r06_kernel_resources.csv")
    lines = open(path).read().splitlines(keepends=True)
    before = "".join(l for l in lines if "pathvalid" not in l)
    assert hashlib.sha256(before.encode()).hexdigest() == PARENT_LEDGER_SHA256
    rows = _ledger(path)
    mine = [k for k in rows if "pathvalid" in k[1]]
    assert len(mine) == 16 * len(KERNELS) * 2 and {fl for fl, _ in mine} == {"exact", "strict"}
    for fl, ns in (("exact", "pik_exact"), ("strict", "pik_strict")):
        for d in range(1, 17):
            for k in KERNELS:
                r = rows[(fl, f"{ns}::{k}<{d}>")]
                assert int(r["vgpr_spills"]) == 0 and int(r["scratch_bytes_per_lane"]) == 0, (fl, k, d)


def test_retaken_ledger_holds_every_committed_row(pk):
    """what this build's compiler reports is the committed ledger, the rows from before this family included"""
    from pick_ik_amd import build as Bd
    if Bd.ledger_rows() is None:
        pytest.skip("the libraries were not built from objects here (no resource remarks)")
    retaken = _ledger(Bd.write_ledger())
    committed = _ledger(os.path.join(ROOT, "profiles", "r06_kernel_resources.csv"))
    assert set(retaken) == set(committed)
    for k, r in committed.items():
        assert retaken[k] == r, k


def test_flavour_hashes_are_the_parents():
    from pick_ik_amd import build as Bd
    assert {ns: Bd.flavour_sha(ns) for ns in Bd.FLAVOUR_FLAGS} == PARENT_FLAVOUR_SHA
