"""pikamd_validity_batch on the GPU: valid, clearance and centres of a sphere model equal the normative numpy code of
tests/validity_reference.py at tolerance zero -- fed by pikamd_fk_batch of the cut-chain handles (the definition) and by
the CPU oracle's forward kinematics of the same chains -- on the Panda with a ragged last wavefront and on one generated
chain per length 1..16; the `_device` form equals the host form; every refusal of include/pick_ik_amd.h."""
import ctypes as C
import dataclasses

import numpy as np
import pytest

import pick_ik_amd as pk
from pick_ik_amd import robots, solver
from tests import validity_reference as V
from tests.hip_buffers import DeviceBuffers

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def O(oracle_mod):
    import __graft_entry__ as g
    g.build()
    return oracle_mod


def check(O, ch, model, q, what):
    """the three outputs of a handle of `ch` against the reference over the cut-chain handles and over the oracle"""
    s = pk.Solver(ch, device=0, strict=True)
    fk_of = V.handle_fk_of(lambda c: pk.Solver(c, device=0, strict=True), ch)
    try:
        s.set_validity_model(*model)
        ok, cl, cen = s.validity(q, centres=True)
        with O.math_mode("portable"):
            refs = {"cut-chain handles": V.centres(fk_of, model, q), "oracle": V.centres(V.oracle_fk_of(O, ch), model, q)}
        for name, want in refs.items():
            np.testing.assert_array_equal(cen, want, err_msg=f"{what}: centres vs {name}")
            np.testing.assert_array_equal(cl, V.clearance(model, want), err_msg=f"{what}: clearance vs {name}")
            np.testing.assert_array_equal(ok, V.valid(model, want), err_msg=f"{what}: valid vs {name}")
        ok2, cl2 = s.validity(q)
        np.testing.assert_array_equal(ok2, ok)
        np.testing.assert_array_equal(cl2, cl)
        return ok, cl, cen
    finally:
        V.close_all(fk_of)
        s.close()


def test_panda_model_equals_the_reference(O, exact_flavour):
    ch = robots.panda()
    model = robots.panda_spheres()
    rng = np.random.default_rng(3)
    n = 130  # (two full wavefronts and a tail of two lanes)
    q = rng.uniform(ch.qmin, ch.qmax, size=(n, 7))
    q[0] = robots.PANDA_HOME
    q[1, 2] = np.nan
    ok, cl, cen = check(O, ch, model, q, f"panda [{exact_flavour}]")
    assert ok[0] and cl[0] > 0.0 and ok[1]
    assert ok[2:].any() and (~ok[2:]).any(), "the random candidates are on both sides of the test"


def generated_chain(d, prismatic=()):
    """a chain of d joints: origins with arbitrary, axis-aligned and identity transforms, axes of every kind"""
    rng = np.random.default_rng(100 + d)
    origins = np.zeros((d, 6))
    origins[:, :3] = rng.uniform(-0.3, 0.3, size=(d, 3))
    origins[:, 3:] = rng.uniform(-np.pi, np.pi, size=(d, 3))
    axes = rng.normal(size=(d, 3))
    for j in range(d):
        if j % 4 == 1:
            origins[j, 3:] = [np.pi / 2, 0.0, 0.0]
            axes[j] = [0.0, 0.0, 1.0]
        if j % 4 == 2:
            axes[j] = np.eye(3)[j % 3]
        if j % 5 == 3:
            origins[j] = 0.0  # (an identity origin: skipped by the chain product)
    jt = np.array([robots.PRISMATIC if j in prismatic else robots.REVOLUTE for j in range(d)], dtype=np.int32)
    return robots._chain(f"generated{d}", origins, axes, [0.05, -0.02, 0.1, 0.3, -0.2, 0.1], [-2.0] * d, [2.0] * d, [1.0] * d,
                         joint_type=jt)


@pytest.mark.parametrize("d", range(1, 17))
def test_generated_chains_equal_the_reference(O, exact_flavour, d):
    """three link spheres (behind the first, the middle and the last variable; the middle one at its frame's origin)
    and one fixed sphere; the chain of six joints has prismatic ones"""
    ch = generated_chain(d, prismatic=(1, 4) if d == 6 else ())
    spheres = [(d - 1, (0.1, -0.05, 0.2), 0.1), (-1, (0.3, 0.2, 0.4), 0.25), ((d - 1) // 2, (0.0, 0.0, 0.0), 0.15),
               (0, (-0.1, 0.0, 0.05), 0.05)]
    pairs = np.array([[0, 1], [2, 1], [3, 1], [0, 3], [0, 2]], dtype=np.int32)
    rng = np.random.default_rng(d)
    q = rng.uniform(-2.0, 2.0, size=(64, d))
    ok, cl, cen = check(O, ch, (spheres, pairs), q, f"generated chain of {d} [{exact_flavour}]")
    assert np.isfinite(cl).all()


@pytest.mark.parametrize("exact", [None, False], ids=["default_exact", "fast"])
def test_every_handle_gets_the_same_arithmetic_and_the_device_form_equals_the_host_form(O, exact):
    ch = robots.panda()
    model = robots.panda_spheres()
    rng = np.random.default_rng(4)
    n = 70
    q = rng.uniform(ch.qmin, ch.qmax, size=(n, 7))
    ref = pk.Solver(ch, device=0, exact=True)
    s = pk.Solver(ch, device=0, exact=exact)
    d = None
    try:
        ref.set_validity_model(*model)
        s.set_validity_model(*model)
        want = ref.validity(q, centres=True)
        for x, y, w in zip(s.validity(q, centres=True), want, ("valid", "clearance", "centres")):
            np.testing.assert_array_equal(x, y, err_msg=f"exact={exact}: {w}")
        d = DeviceBuffers()
        ns = len(model[0])
        dq, dv, dc, dcen = d.upload(q), d.alloc(4 * n), d.alloc(8 * n), d.alloc(8 * 3 * ns * n)
        s.validity_device(n, dq, dv, dc, dcen)
        d.sync()
        np.testing.assert_array_equal(d.download(dv, n, np.int32) != 0, want[0])
        np.testing.assert_array_equal(d.download(dc, n, np.float64), want[1])
        np.testing.assert_array_equal(d.download(dcen, (n, ns, 3), np.float64), want[2])
        dv2 = d.alloc(4 * n)
        s.validity_device(n, dq, dv2)  # (clearance and centres may be NULL)
        d.sync()
        np.testing.assert_array_equal(d.download(dv2, n, np.int32) != 0, want[0])
        # a model without pairs: valid and +infinity everywhere; a new model replaces the old one
        s.set_validity_model(model[0], np.zeros((0, 2), dtype=np.int32))
        ok, cl, cen = s.validity(q, centres=True)
        assert ok.all() and np.isposinf(cl).all()
        np.testing.assert_array_equal(cen, want[2])
        s.set_validity_model(*model)
        np.testing.assert_array_equal(s.validity(q)[1], want[1])
        assert s.validity(q[:0])[0].shape == (0,)
    finally:
        if d is not None:
            d.free()
        s.close()
        ref.close()


def raw_model(spheres, pairs, n_spheres=None, n_pairs=None, null_spheres=False, null_pairs=False):
    sph = [solver.Sphere(*sp) for sp in spheres]
    arr = (solver.Sphere * max(1, len(sph)))(*sph)
    pr = np.ascontiguousarray(np.asarray(pairs, dtype=np.int32).reshape(-1, 2))
    m = solver.ValidityModel(len(sph) if n_spheres is None else n_spheres, None if null_spheres else arr,
                             pr.shape[0] if n_pairs is None else n_pairs,
                             None if null_pairs else pr.ctypes.data_as(C.POINTER(C.c_int32)))
    m._keep = (arr, pr)
    return m


def test_refusals(O):
    EINVAL, EUNSUPPORTED = -1, -4
    ch = robots.panda()
    s = pk.Solver(ch, device=0)
    L, h = s._L, s._h
    err = lambda: L.pikamd_last_error().decode()
    setm = lambda m: L.pikamd_set_validity_model(h, C.byref(m))
    good = [(0, (0.0, 0.0, 0.1), 0.1), (-1, (0.5, 0.0, 0.5), 0.1), (6, (0.0, 0.0, 0.0), 0.0)]
    pairs = [[0, 1], [2, 1]]
    dp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int32)
    try:
        q = np.tile(robots.PANDA_HOME, (4, 1))
        valid = np.zeros(4, dtype=np.int32)
        call = lambda n=4, qq=q, vv=valid: L.pikamd_validity_batch(h, n, None if qq is None else qq.ctypes.data_as(dp),
                                                                   None if vv is None else vv.ctypes.data_as(ip), None, None)
        # without a model
        assert call() == EINVAL and "no validity model" in err()
        assert L.pikamd_validity_batch_device(h, 4, None, None, None, None, None) == EINVAL
        # counts, NULL arrays
        assert setm(raw_model(good, pairs)) == 0
        for bad in (dict(n_spheres=-1), dict(n_spheres=33), dict(n_pairs=-1), dict(n_pairs=257)):
            assert setm(raw_model(good, pairs, **bad)) == EINVAL and "expected 0.." in err(), bad
        assert setm(raw_model(good, pairs, null_spheres=True)) == EINVAL and "NULL" in err()
        assert setm(raw_model(good, pairs, null_pairs=True)) == EINVAL and "NULL" in err()
        assert setm(raw_model([], [], null_spheres=True, null_pairs=True)) == 0  # (nothing is needed of an empty model)
        # spheres
        for bad in ((0, (np.nan, 0, 0), 0.1), (0, (0, np.inf, 0), 0.1), (0, (0, 0, 0), np.nan), (0, (0, 0, 0), np.inf),
                    (0, (0, 0, 0), -0.1)):
            assert setm(raw_model([bad] + good[1:], pairs)) == EINVAL and "finite" in err(), bad
        for after in (-2, 7, 100):
            assert setm(raw_model([(after, (0, 0, 0), 0.1)] + good[1:], pairs)) == EINVAL and "after_variable" in err(), after
        # pairs
        for bad in ([0, 3], [-1, 0], [1, 1]):
            assert setm(raw_model(good, [bad])) == EINVAL and "pair" in err(), bad
        # a refused model leaves the handle's model as it was
        assert setm(raw_model(good, pairs)) == 0 and call() == 0
        assert setm(raw_model(good, [[1, 1]])) == EINVAL and call() == 0
        # the call itself
        assert call(n=-1) == EINVAL and "n >= 0" in err()
        assert call(qq=None) == EINVAL and "NULL" in err()
        assert call(vv=None) == EINVAL and "NULL" in err()
        assert call(n=0, qq=None, vv=None) == 0
        s.set_option("joint_layout", "soa")
        assert call() == EINVAL and "joint_layout soa" in err()
        s.set_option("joint_layout", "aos")
        assert call() == 0
        # NULL: no model again
        assert L.pikamd_set_validity_model(h, None) == 0 and call() == EINVAL
        s.set_validity_model(good, pairs)
        assert call() == 0
        s.clear_validity_model()
        assert call() == EINVAL
        assert L.pikamd_set_validity_model(None, None) == EINVAL
    finally:
        s.close()
    # a planar joint: only its theta slot names a link
    planar = dataclasses.replace(generated_chain(5), joint_type=np.array(
        [robots.REVOLUTE, robots.PLANAR_X, robots.PLANAR_Y, robots.PLANAR_THETA, robots.REVOLUTE], dtype=np.int32))
    s = pk.Solver(planar, device=0)
    try:
        for after in (1, 2):
            with pytest.raises(pk.PickIkAmdError, match="planar"):
                s.set_validity_model([(after, (0, 0, 0), 0.1), (-1, (1, 0, 0), 0.1)], [[0, 1]])
        s.set_validity_model([(3, (0.1, 0, 0), 0.1), (0, (0, 0, 0.1), 0.1), (-1, (1, 0, 0), 0.1)], [[0, 2], [1, 2]])
        assert s.validity(np.zeros((2, 5)))[0].shape == (2,)
    finally:
        s.close()
    # what the test cannot walk: several tip frames, a floating joint, mimic joints
    one = [(0, (0, 0, 0), 0.1), (-1, (1, 0, 0), 0.1)]
    for chain in (robots.torso_dual_arm(), robots.floating_panda(),
                  dataclasses.replace(robots.panda(), mimic=(robots.MimicJoint(6, 6, (0, 0, 0.05, 0, 0, 0), (0, 0, 1)),))):
        s = pk.Solver(chain, device=0)
        try:
            with pytest.raises(pk.PickIkAmdError, match="error -4"):
                s.set_validity_model(one, [[0, 1]])
        finally:
            s.close()
    assert EUNSUPPORTED == -4
