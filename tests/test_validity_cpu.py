"""The sphere validity test without a GPU (pikamd_set_validity_model, pikamd_validity_batch, the validity step of both
restart searches): the normative numpy code of tests/validity_reference.py on chains whose centres are known in closed
form and over the CPU oracle's forward kinematics of the cut chains; the declarations and the bindings; and the
CONDITIONS the fixture of the GPU tests (the Panda of search_reference, robots.panda_spheres) has to meet, asserted on
the loops over the oracle -- tests/test_gpu_search_validity.py asserts them again on what the GPU returns."""
import ctypes as C
import math
import os
import re
import subprocess

import numpy as np
import pytest

from pick_ik_amd import robots
from tests import gate_reference as GT
from tests import search_reference as SR
from tests import validity_reference as V

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "pick_ik_amd.h")
B = 64


@pytest.fixture(params=["portable", "fma"])
def mode(request):
    return request.param


def rr_model():
    """the elbow and the tip of the 2 + 1 arm, a sphere at the shoulder (the link frame's origin) and two obstacles"""
    spheres = [(0, (2.0, 0.0, 0.0), 0.25), (1, (1.0, 0.0, 0.0), 0.25), (0, (0.0, 0.0, 0.0), 0.5), (-1, (0.0, 3.5, 0.0), 0.25),
               (-1, (-4.0, 0.0, 1.0), 0.5)]
    return spheres, np.array([[1, 3], [0, 3], [1, 4], [2, 4]], dtype=np.int32)


def test_centres_of_the_planar_arm_in_closed_form(oracle_mod, mode):
    O = oracle_mod
    ch = robots.rr()
    model = rr_model()
    q = np.array([[0.0, 0.0], [math.pi / 2, 0.0], [math.pi / 2, math.pi / 2], [0.0, -math.pi / 2], [math.pi, 0.0]])
    want = np.array([[[2, 0, 0], [3, 0, 0]], [[0, 2, 0], [0, 3, 0]], [[0, 2, 0], [-1, 2, 0]], [[2, 0, 0], [2, -1, 0]],
                     [[-2, 0, 0], [-3, 0, 0]]], dtype=np.float64)
    with O.math_mode(mode):
        cen = V.centres(V.oracle_fk_of(O, ch), model, q)
    assert cen.shape == (5, 5, 3)
    np.testing.assert_array_equal(cen[0, :2], want[0])          # (q = 0: nothing to round)
    np.testing.assert_allclose(cen[:, :2], want, rtol=0, atol=1e-15)
    np.testing.assert_array_equal(cen[:, 2], np.zeros((5, 3)))  # the shoulder does not move
    np.testing.assert_array_equal(cen[:, 3], np.broadcast_to([0.0, 3.5, 0.0], (5, 3)))  # copied
    cl = V.clearance(model, cen)
    ok = V.valid(model, cen)
    # straight up (q = (pi/2, 0)): the tip is 0.5 from the obstacle at (0, 3.5, 0) up to the rounding of cos(pi/2), the
    # radii add up to 0.5 -- touching, to an ulp or two of 3.0 either way
    assert abs(cl[1]) < 1e-15
    # q = 0: the nearest pair is the shoulder and the far obstacle, neither of which moves
    assert cl[0] == math.sqrt(17.0) - 1.0 and (cl <= cl[0]).all()
    assert ok[0] and ok[3]


def test_touching_spheres_are_valid_and_a_nan_does_not_trip_the_test():
    """on hand-made centres: clear_m = 0.0 exactly is valid, the next double below is not; a NaN never replaces the
    clearance and refuses nothing; no pair: valid, +infinity"""
    spheres = [(-1, (0, 0, 0), 1.0), (-1, (0, 0, 0), 2.0), (-1, (0, 0, 0), 0.5)]
    pairs = np.array([[0, 1], [0, 2]], dtype=np.int32)
    model = (spheres, pairs)
    cen = np.zeros((4, 3, 3))
    cen[:, 1, 0] = [3.0, np.nextafter(3.0, 0.0), 3.0, np.nan]  # sphere 1 along x: touching, overlapping, ...
    cen[:, 2, 2] = [5.0, 5.0, np.nan, 1.0]                     # sphere 2 along z
    cl, ok = V.clearance(model, cen), V.valid(model, cen)
    np.testing.assert_array_equal(ok, [True, False, True, False])
    assert cl[0] == 0.0 and cl[1] < 0.0 and cl[2] == 0.0 and cl[3] == -0.5
    empty = (spheres, np.zeros((0, 2), dtype=np.int32))
    assert V.valid(empty, cen).all() and np.isinf(V.clearance(empty, cen)).all()


def test_a_nan_joint_value_is_valid(oracle_mod, mode):
    O = oracle_mod
    ch = robots.panda()
    model = robots.panda_spheres()
    q = np.tile(robots.PANDA_HOME, (3, 1))
    q[1, 0] = np.nan   # every moving sphere is nowhere: only NaN clearances
    q[2, 6] = np.nan   # the last link's two spheres
    with O.math_mode(mode):
        cen = V.centres(V.oracle_fk_of(O, ch), model, q)
    cl, ok = V.clearance(model, cen), V.valid(model, cen)
    assert ok[0] and ok[1] and ok[2] and np.isinf(cl[1]) and np.isfinite(cl[0]) and cl[0] > 0.0
    assert np.isnan(cen[1, 1:9]).all() and not np.isnan(cen[2, :7]).any()


def test_centres_over_the_oracle_are_the_cut_chains_positions(oracle_mod, mode):
    """the definition, spelt out once: sphere k of the Panda model is where the oracle puts the tip of the chain cut
    behind its variable; the flange sphere (all-zero centre) is the last joint's frame origin"""
    O = oracle_mod
    ch = robots.panda()
    spheres, pairs = robots.panda_spheres()
    rng = np.random.default_rng(5)
    q = rng.uniform(ch.qmin, ch.qmax, size=(16, 7))
    with O.math_mode(mode):
        cen = V.centres(V.oracle_fk_of(O, ch), (spheres, pairs), q)
        for k, (after, c, _r) in enumerate(spheres):
            if after >= 0:
                want = O.Oracle(robots.cut_chain(ch, after, c)).fk(np.ascontiguousarray(q[:, :after + 1]))[:, :3]
                np.testing.assert_array_equal(cen[:, k], want)
        full = O.Oracle(robots.cut_chain(ch, 6, (0.0, 0.0, 0.0))).fk(q)[:, :3]
    np.testing.assert_array_equal(cen[:, 8], full)
    assert len(pairs) <= 256 and len(spheres) <= 32 and (pairs[:, 0] != pairs[:, 1]).all()
    assert V.valid((spheres, pairs), cen[:0]).shape == (0,)


FAMILIES = {"local": (GT.K, dict(GT.PANDA_KW)), "global": (GT.K_GLOBAL, dict(GT.PANDA_KW, **GT.GLOBAL_KW))}


def oracle_loops(O, family, gate, model, **kw):
    ch, goals, seed, _ = SR.fixture("panda", lambda c: O.Oracle(c).fk, B)
    K, params = FAMILIES[family]
    loop = V.oracle_search if family == "local" else V.oracle_search_global
    return loop(O, ch, goals, seed, K, params, gate, model, rng_seed=SR.RNG_SEED, all_attempts=True, **kw), seed


def check_fixture_conditions(plain, got, gated, what=""):
    """the conditions of the issue, on a call's outputs without the model (plain) and with it (got)"""
    refused0, valid0, rescued, ended = V.fixture_counts(plain[6], got[6], got[1], got[4])
    both = int(((plain[6] > 0) & (got[6] == V.VALIDITY_REFUSED)).sum())
    print(f"{what}: refused at attempt 0 / valid at attempt 0 / rescued after a refusal / ending refused = "
          f"{refused0}/{valid0}/{rescued}/{ended}; rows the gate passes and the test refuses: {both}")
    assert refused0 >= 8 and valid0 >= 8 and rescued >= 2 and ended >= 1, (what, refused0, valid0, rescued, ended)
    if gated:
        assert both >= 1, what


@pytest.mark.parametrize("gate", [None, GT.PANDA_GATE], ids=["no_gate", "gate"])
@pytest.mark.parametrize("family", ["local", "global"])
def test_fixture_conditions_on_the_oracle_loops(oracle_mod, mode, family, gate):
    O = oracle_mod
    model = robots.panda_spheres()
    with O.math_mode(mode):
        plain, seed = oracle_loops(O, family, gate, None)
        got, _ = oracle_loops(O, family, gate, model)
        none, _ = oracle_loops(O, family, gate, (model[0], np.zeros((0, 2), dtype=np.int32)))
    check_fixture_conditions(plain, got, gate is not None, f"[{mode}] {family} {'gated' if gate else 'no gate'}")
    # a refused answer is the seed, its cost stays; a model without pairs refuses nothing
    refused = got[1] == V.VALIDITY_REFUSED
    np.testing.assert_array_equal(got[0][refused], seed[refused])
    for x, y in zip(none, plain):
        np.testing.assert_array_equal(x, y)
    # the rows in front of the first refusal are the plain loop's
    first = np.array([np.argmax(got[6][b] == V.VALIDITY_REFUSED) if (got[6][b] == V.VALIDITY_REFUSED).any() else got[6].shape[1]
                      for b in range(B)])
    for b in range(B):
        np.testing.assert_array_equal(got[6][b, :first[b]], plain[6][b, :first[b]])


def test_header_and_bindings_declare_the_model():
    header = open(HEADER).read()
    begin, end = header.index("[host-api-begin]"), header.index("[host-api-end]")
    for name in ("pikamd_set_validity_model", "pikamd_validity_batch", "pikamd_validity_batch_device"):
        m = re.search(r"\b" + name + r"\s*\(", header)
        assert m and begin < m.start() < end, name
    for text in (r"#define\s+PIKAMD_VALIDITY_REFUSED\s+\(-1004\)", r"#define\s+PIKAMD_MAX_SPHERES\s+32\b",
                 r"#define\s+PIKAMD_MAX_SPHERE_PAIRS\s+256\b", r"typedef struct pikamd_sphere\b",
                 r"typedef struct pikamd_validity_model\b"):
        m = re.search(text, header)
        assert m and begin < m.start() < end, text
    from pick_ik_amd import solver
    assert solver.VALIDITY_REFUSED == V.VALIDITY_REFUSED == -1004
    assert (solver.MAX_SPHERES, solver.MAX_SPHERE_PAIRS) == (32, 256)
    for name in ("pikamd_set_validity_model", "pikamd_validity_batch", "pikamd_validity_batch_device"):
        assert name in solver.EXPORTED_SYMBOLS
    for method in ("set_validity_model", "clear_validity_model", "validity", "validity_device"):
        assert callable(getattr(solver.Solver, method))


def test_ctypes_structs_match_the_header(tmp_path):
    from pick_ik_amd import solver
    src = tmp_path / "sizes.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "pick_ik_amd.h"\n'
                   'int main(void) { printf("%zu %zu %zu %zu %zu %zu %zu %zu\\n", sizeof(pikamd_sphere), '
                   'offsetof(pikamd_sphere, centre), offsetof(pikamd_sphere, radius), sizeof(pikamd_validity_model), '
                   'offsetof(pikamd_validity_model, spheres), offsetof(pikamd_validity_model, n_pairs), '
                   'offsetof(pikamd_validity_model, pairs), offsetof(pikamd_sphere, reserved)); return 0; }\n')
    exe = tmp_path / "sizes"
    subprocess.run(["gcc", "-I" + os.path.dirname(HEADER), str(src), "-o", str(exe)], check=True)
    got = [int(v) for v in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    S, M = solver.Sphere, solver.ValidityModel
    assert got == [C.sizeof(S), S.centre.offset, S.radius.offset, C.sizeof(M), M.spheres.offset, M.n_pairs.offset,
                   M.pairs.offset, S.reserved.offset]
    s = S(3, (0.1, 0.2, 0.3), 0.5)
    assert (s.after_variable, s.reserved, list(s.centre), s.radius) == (3, 0, [0.1, 0.2, 0.3], 0.5)


def test_the_validity_kernels_are_a_family_of_their_own():
    from pick_ik_amd import build as Bd
    assert Bd.FAMILIES["pik_validity_inst.hip"] == (("exact",), ("strict",))
    app = Bd.APPENDED_FAMILIES
    assert app.index("pik_validity_inst.hip") < app.index("pik_globalpath_inst.hip") == len(app) - 1
    for strict in (False, True):
        objs = [o for o in Bd.link_objects(strict) if o[1] == "pik_validity_inst.hip"]
        assert len(objs) == 16 and all("-ffp-contract=off" in Bd._cmd(*o, strict) for o in objs)
    # the test's arithmetic is compiled where fk's chain product is: nothing of it for the fast flavours
    text = open(os.path.join(Bd.CSRC, "pik_validity.hpp")).read()
    assert "#if !defined(PIK_STRICT)\n#error" in text
    for inst in ("pik_inst.hip", "pik_launch.hpp", "pik_kernels.hpp", "pik_math.hpp", "pik_solver.hpp"):
        assert "pik_validity" not in open(os.path.join(Bd.CSRC, inst)).read(), inst
