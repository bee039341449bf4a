"""Normal perturbation (include/rtc.h rtc_bump), the parts that need no GPU: a scalar-numpy restatement of steps 1-4 of the rule, with
the ORACLE's noise, against rtc_bump_normal bit for bit; the limits (through C where the library checks them before it needs a device,
and through the Python classes and the rtw setter); the refusals of the oracle, the emulator and the flatten helpers; the exports, the
Rust mirror and the build tables."""
import ctypes as C
import itertools
import math
import os

import numpy as np
import pytest

import foreign_flattener as ff
from raytracer_challenge_amd.cabi import RtcBump, RtcBumpInfo, load
from raytracer_challenge_amd.backend import RtwError
from raytracer_challenge_amd.scene import (Bump, Camera, Color, Element, Material, Matrix, Pattern, PointLight, ShapeArgs, Vector, World)
from test_shim_layout import c_struct, rust_struct

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "raytracer_challenge_amd", "csrc", "librtc_amd.so")
vp = C.c_void_p
SIMPLEX, FRACTAL, RIPPLE = 0, 1, 2
MAX_OCTAVES = 64


def same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a, dtype=np.float64).view(np.uint64), np.ascontiguousarray(b, dtype=np.float64).view(np.uint64))


# ---- the restatement of steps 1-4 (shared with test_bump_gpu.py): numpy float64 scalars, one operation at a time, the oracle's noise ----
def restated_normal(orc, kind, octaves, a, f, m, X, n):
    """include/rtc.h rtc_bump, steps 1-4.  m: 16 floats, row-major material_inv; X: the point; n: the unit normal before the flip."""
    F = np.float64
    m = [F(v) for v in m]
    x, y, z = (F(v) for v in X)
    n = [F(v) for v in n]
    a, f = F(a), F(f)
    with np.errstate(all="ignore"):
        q = [((m[4 * r] * x + m[4 * r + 1] * y) + m[4 * r + 2] * z) + m[4 * r + 3] * F(1.0) for r in range(3)]
        sx, sy, sz = q[0] * f, q[1] * f, q[2] * f
        if kind == RIPPLE:
            r = np.sqrt(sx * sx + sz * sz)
            if r == 0.0:
                d = [F(0.0), F(0.0), F(0.0)]
            else:
                g = F(2.0) * (r - np.floor(r))
                w = F(1.0) - F(2.0) * g if g < 1.0 else F(2.0) * g - F(3.0)
                d = [(sx / r) * w, F(0.0), (sz / r) * w]
        else:
            noise = (lambda u, v, t: F(orc.lib.orc_simplex(u, v, t))) if kind == SIMPLEX else (lambda u, v, t: F(orc.lib.orc_fractal(u, v, t, octaves)))
            d = [noise(sx, sy, sz), noise(sx, sy, sz + F(1.0)), noise(sx, sy, sz + F(2.0))]
        g = [(m[c] * d[0] + m[4 + c] * d[1]) + m[8 + c] * d[2] for c in range(3)]
        v = [n[c] + a * g[c] for c in range(3)]
        if v[0] == n[0] and v[1] == n[1] and v[2] == n[2]:
            return np.array(n)
        mag = np.sqrt((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2])
        return np.array([v[0] / mag, v[1] / mag, v[2] / mag])


def lib_normal(lib, kind, octaves, a, f, m, X, n, expect=0):
    b = RtcBump(0, kind, octaves, 0, a, f)
    out = (C.c_double * 3)()
    rc = lib.rtc_bump_normal(C.byref(b), (C.c_double * 16)(*m), (C.c_double * 3)(*X), (C.c_double * 3)(*n), out)
    assert rc == expect, lib.rtc_last_error()
    return np.array(list(out))


def matrices():
    return {
        "identity": Matrix.id(),
        "scale": Matrix.scaling(2.0, 0.25, 7.5),
        "shear": Matrix.shearing(0.5, -0.25, 0.125, 1.5, -2.0, 0.75),
        "translation": Matrix.translation(3.5, -1.25, 0.1),
        "all": Matrix.translation(0.3, 2.0, -1.0) * Matrix.rotation_y(0.7) * Matrix.shearing(0.1, 0.0, 0.0, 0.2, 0.0, 0.0) * Matrix.scaling(1.5, 0.5, 3.0),
    }


def unit(v):
    v = np.asarray(v, dtype=np.float64)
    return v / np.sqrt((v * v).sum())


def test_restated_rule_is_rtc_bump_normal_bit_for_bit(orc):
    lib = load(LIB)
    rng = np.random.default_rng(2026)
    n_checked = 0
    moved = 0
    for (mname, M), mag in itertools.product(matrices().items(), (1e-3, 0.1, 1.0, 37.5, 1e3)):
        m = ff.inverse(M).flat()
        for kind, octaves in ((SIMPLEX, 0), (FRACTAL, 1), (FRACTAL, 3), (FRACTAL, 8), (RIPPLE, 0)):
            for a in (0.0, 0.05, 1.0, 10.0):
                X = rng.normal(size=3) * mag
                n = unit(rng.normal(size=3))
                f = float(rng.choice([0.1, 1.0, 2.5, 40.0]))
                want = restated_normal(orc, kind, octaves, a, f, m, X, n)
                got = lib_normal(lib, kind, octaves, a, f, m, X, n)
                assert same_bits(got, want), (mname, mag, kind, octaves, a, f, X, n, got, want)
                if a == 0.0:
                    assert same_bits(got, n)
                else:
                    moved += int(not same_bits(got, n))
                    assert abs(np.sqrt((got * got).sum()) - 1.0) < 4e-16
                n_checked += 1
    assert n_checked == 5 * 5 * 5 * 4 and moved > 0.9 * n_checked * 3 / 4     # the records do move the normal


def test_fractal_with_one_octave_is_simplex_and_the_noise_is_the_oracles(orc):
    lib = load(LIB)
    m = Matrix.id().flat()
    for X in ((0.3, 1.7, -2.2), (12.5, -0.01, 3.0)):
        n = unit((0.2, 1.0, -0.4))
        assert same_bits(lib_normal(lib, FRACTAL, 1, 0.3, 1.0, m, X, n), lib_normal(lib, SIMPLEX, 0, 0.3, 1.0, m, X, n))
        # amplitude 1 on the zero normal hands out normalize(g) = normalize(d) under the identity: the library's noise is the oracle's
        d = np.array([orc.lib.orc_simplex(X[0], X[1], X[2] + k) for k in (0.0, 1.0, 2.0)])
        assert same_bits(lib_normal(lib, SIMPLEX, 0, 1.0, 1.0, m, X, (0.0, 0.0, 0.0)), d / np.sqrt((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]))


def test_ripple_edges(orc):
    lib = load(LIB)
    m = Matrix.id().flat()
    n = (0.0, 1.0, 0.0)
    cases = {
        "r == 0": (0.0, 0.0, 0.0), "on the y axis": (0.0, 3.25, 0.0), "on the y axis, below": (-0.0, -7.0, 0.0),
        "g == 0 (r an integer)": (3.0, 0.5, 4.0), "g == 0, r == 1": (1.0, 0.0, 0.0), "g == 1 (r a half)": (1.5, 2.0, 0.0), "g == 1, on z": (0.0, 0.0, -2.5),
        "between": (0.3, 0.0, 0.4), "far": (300.0, 1.0, -400.25),
    }
    for why, X in cases.items():
        for a in (0.05, 1.0):
            want = restated_normal(orc, RIPPLE, 0, a, 1.0, m, X, n)
            assert same_bits(lib_normal(lib, RIPPLE, 0, a, 1.0, m, X, n), want), why
    one = lambda X: lib_normal(lib, RIPPLE, 0, 1.0, 1.0, m, X, n)  # noqa: E731
    assert same_bits(one((0.0, 0.0, 0.0)), n) and same_bits(one((0.0, 3.25, 0.0)), n)          # d = 0: the normal's own bits
    # g == 0: w = 1, the slope points outward; g == 1: w = -1, inward; v = n + d, normalised
    assert same_bits(one((1.0, 0.0, 0.0)), np.array([1.0, 1.0, 0.0]) / np.sqrt(2.0))
    assert same_bits(one((1.5, 2.0, 0.0)), np.array([-1.0, 1.0, 0.0]) / np.sqrt(2.0))
    assert same_bits(one((3.0, 0.5, 4.0)), unit((0.6, 1.0, 0.8)))
    # g == 0.5 (r = 0.25): w = 0: a flat spot, and the normal keeps its bits
    assert same_bits(one((0.25, 0.0, 0.0)), n)
    # the frequency scales the point, not the slope
    assert same_bits(lib_normal(lib, RIPPLE, 0, 1.0, 4.0, m, (0.25, 0.0, 0.0), n), one((1.0, 0.0, 0.0)))


def test_nan_and_infinite_points_give_what_ieee_gives(orc):
    lib = load(LIB)
    nan, inf = math.nan, math.inf
    n = unit((0.0, 1.0, 1.0))
    for M in (Matrix.id(), Matrix.scaling(2.0, 3.0, 0.5)):
        m = ff.inverse(M).flat()
        for X in ((nan, 0.0, 1.0), (1.0, nan, 2.0), (inf, 1.0, 0.0), (0.5, -inf, 0.5), (1.0, 2.0, inf), (inf, nan, -inf), (1e308, 1e308, -1e308)):
            for kind, octaves in ((SIMPLEX, 0), (FRACTAL, 3), (RIPPLE, 0)):
                got, want = lib_normal(lib, kind, octaves, 0.5, 1.0, m, X, n), restated_normal(orc, kind, octaves, 0.5, 1.0, m, X, n)
                assert np.array_equal(np.isnan(got), np.isnan(want)), (X, kind)
                assert same_bits(np.where(np.isnan(got), 0.0, got), np.where(np.isnan(want), 0.0, want)), (X, kind)
    # a NaN normal stays NaN whatever the record says
    assert np.isnan(lib_normal(lib, RIPPLE, 0, 0.5, 1.0, Matrix.id().flat(), (0.3, 0.0, 0.4), (nan, 1.0, 0.0))).any()


def test_amplitude_zero_returns_the_normals_own_bits(orc):
    """... for a normal whose length is one rounding off 1 as well: no renormalisation happens."""
    lib = load(LIB)
    rng = np.random.default_rng(7)
    m = ff.inverse(matrices()["all"]).flat()
    normals = [unit(rng.normal(size=3)) for _ in range(40)]
    normals += [np.array([1.0, 0.0, 0.0]), np.array([-0.0, 0.0, -1.0]), np.array([np.nextafter(1.0, 2.0), 0.0, 0.0]), np.array([np.nextafter(1.0, 0.0), 0.0, 0.0]),
                np.array([0.6, np.nextafter(0.8, 1.0), 0.0]), np.array([0.0, 0.0, 0.0]), np.array([3.0, -4.0, 12.0])]
    off_one = sum(1 for v in normals if ((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2]) != 1.0)
    assert off_one >= 5
    for v in normals:
        for kind, octaves in ((SIMPLEX, 0), (FRACTAL, 8), (RIPPLE, 0)):
            for a in (0.0, -0.0):
                assert same_bits(lib_normal(lib, kind, octaves, a, 2.0, m, (0.3, 1.7, -2.2), v), v)
                assert same_bits(restated_normal(orc, kind, octaves, a, 2.0, m, (0.3, 1.7, -2.2), v), v)


# ---- limits -----------------------------------------------------------------------------------------------------------------------
def two_material_world():
    red = Material(pattern=Pattern.plain(Color(0.9, 0.2, 0.2)))
    return World([PointLight(Color.white(), Vector.point(0, 5, 0))],
                 [Element.plane(ShapeArgs()), Element.sphere(ShapeArgs(material=red, transform=Matrix.translation(0, 1, 0)))])


def bad_records(n_materials):
    nan, inf = math.nan, math.inf
    ok = RtcBump(0, SIMPLEX, 0, 0, 0.05, 2.0)
    return {
        "material index one past the end": [RtcBump(n_materials, SIMPLEX, 0, 0, 0.05, 2.0)],
        "a huge material index": [RtcBump(2 ** 32 - 1, RIPPLE, 0, 0, 0.05, 2.0)],
        "two records on one material": [ok, RtcBump(1, RIPPLE, 0, 0, 0.1, 1.0), RtcBump(0, FRACTAL, 2, 0, 0.05, 2.0)],
        "unknown kind": [RtcBump(0, 3, 0, 0, 0.05, 2.0)],
        "negative kind": [RtcBump(0, -1, 0, 0, 0.05, 2.0)],
        "NaN amplitude": [RtcBump(0, SIMPLEX, 0, 0, nan, 2.0)],
        "infinite amplitude": [RtcBump(0, RIPPLE, 0, 0, -inf, 2.0)],
        "NaN frequency": [RtcBump(0, SIMPLEX, 0, 0, 0.05, nan)],
        "infinite frequency": [RtcBump(0, SIMPLEX, 0, 0, 0.05, inf)],
        "zero frequency": [RtcBump(0, RIPPLE, 0, 0, 0.05, 0.0)],
        "negative frequency": [RtcBump(0, FRACTAL, 3, 0, 0.05, -1.0)],
        "fractal without octaves": [RtcBump(0, FRACTAL, 0, 0, 0.05, 2.0)],
        "fractal with too many octaves": [RtcBump(0, FRACTAL, MAX_OCTAVES + 1, 0, 0.05, 2.0)],
        "a bad record behind a good one": [ok, RtcBump(1, FRACTAL, 0, 0, 0.05, 2.0)],
    }


def test_limits_through_c_need_no_device():
    """The records' own numbers are validated before the device is looked for: every limit answers RTC_ERR_INVALID (1) here, where valid
    records get as far as RTC_ERR_DEVICE (3) on a machine without one (or succeed on one with)."""
    lib = load(LIB)
    desc = ff.flatten(two_material_world()).desc()
    assert desc.n_materials == 2
    devs = (C.c_int * 1)(0)

    def create(recs, n, multi):
        s = vp()
        rc = (lib.rtc_multi_create_ext4(C.byref(desc), None, None, 0, None, recs, n, devs, 1, C.byref(s)) if multi else
              lib.rtc_scene_create_ext4(C.byref(desc), None, None, 0, None, recs, n, 0, C.byref(s)))
        if rc == 0:
            (lib.rtc_multi_destroy if multi else lib.rtc_scene_destroy)(s)
        return rc
    for multi in (False, True):
        for why, recs in bad_records(desc.n_materials).items():
            arr = (RtcBump * len(recs))(*recs)
            assert create(arr, len(recs), multi) == 1, (why, multi)
            assert b"bump" in lib.rtc_last_error(), why
        assert create(None, 1, multi) == 1 and b"bumps is NULL" in lib.rtc_last_error()       # records announced, none given
        good = (RtcBump * 2)(RtcBump(1, FRACTAL, MAX_OCTAVES, 0, -10.0, 1e-3), RtcBump(0, RIPPLE, 77, 0, 0.0, 1e6))   # (octaves are FRACTAL's alone)
        assert create(good, 2, multi) in (0, 3), lib.rtc_last_error()
        assert create(good, 1, multi) in (0, 3)
        assert create(None, 0, multi) in (0, 3) and create(good, 0, multi) in (0, 3)          # n_bumps == 0 is _ext3
    s = vp()
    assert lib.rtc_scene_create_ext4(None, None, None, 0, None, (RtcBump * 1)(RtcBump(0, SIMPLEX, 0, 0, 0.1, 1.0)), 1, 0, C.byref(s)) == 1   # a NULL descriptor


def test_host_entry_refuses_null_and_bad_records():
    lib = load(LIB)
    m, p, n, o = (C.c_double * 16)(*Matrix.id().flat()), (C.c_double * 3)(1, 2, 3), (C.c_double * 3)(0, 1, 0), (C.c_double * 3)()
    ok = RtcBump(12345, RIPPLE, 0, 0, 0.1, 1.0)                                               # (`material` is not read)
    assert lib.rtc_bump_normal(C.byref(ok), m, p, n, o) == 0
    for args in ((None, m, p, n, o), (C.byref(ok), None, p, n, o), (C.byref(ok), m, None, n, o), (C.byref(ok), m, p, None, o), (C.byref(ok), m, p, n, None)):
        assert lib.rtc_bump_normal(*args) == 1
    for why, recs in bad_records(2).items():
        if "material" in why or "behind" in why:
            continue
        assert lib.rtc_bump_normal(C.byref(recs[0]), m, p, n, o) == 1 and b"bump" in lib.rtc_last_error(), why
    assert lib.rtc_bump_normals(None, None, None, None, 0, None) == 1
    assert lib.rtc_scene_bump_info(None, None) == 1


# ---- the layers -------------------------------------------------------------------------------------------------------------------
def test_bump_and_material_type_errors():
    assert Material().bump is None and Material() == Material(bump=None)                     # existing constructions are unchanged
    b = Bump.simplex(0.05, 2.0)
    assert (b.kind, b.amplitude, b.frequency, b.octaves) == ("simplex", 0.05, 2.0, 0)
    f = Bump.fractal(3, 0.1, 4.0)
    assert (f.kind, f.octaves, f.amplitude, f.frequency) == ("fractal", 3, 0.1, 4.0)
    assert Bump.ripple(-0.2, 0.5).kind == "ripple" and Bump.ripple(0.0, 1).amplitude == 0.0
    assert Material(bump=b).bump is b
    with pytest.raises(Exception):
        b.amplitude = 1.0                                                                      # frozen like the material
    for wrong in ("ripple", 0.05, (0.05, 2.0), Pattern.debug(), 1):
        with pytest.raises(TypeError):
            Material(bump=wrong)
    for wrong in (lambda: Bump("waves", 0.1, 1.0), lambda: Bump.simplex(math.nan, 1.0), lambda: Bump.simplex(math.inf, 1.0), lambda: Bump.ripple(0.1, 0.0),
                  lambda: Bump.ripple(0.1, -2.0), lambda: Bump.ripple(0.1, math.inf), lambda: Bump.fractal(0, 0.1, 1.0), lambda: Bump.fractal(MAX_OCTAVES + 1, 0.1, 1.0)):
        with pytest.raises(ValueError):
            wrong()
    for wrong in (lambda: Bump.simplex("0.1", 1.0), lambda: Bump.simplex(0.1, None), lambda: Bump.fractal(2.5, 0.1, 1.0), lambda: Bump.simplex(True, 1.0)):
        with pytest.raises(TypeError):
            wrong()


def bumped_world(bump=None, bump2=None):
    shared = dict(pattern=Pattern.plain(Color(0.9, 0.2, 0.2)), diffuse=0.7)
    return World([PointLight(Color.white(), Vector.point(0, 5, -3))],
                 [Element.plane(ShapeArgs(material=Material(**shared, bump=bump))),
                  Element.sphere(ShapeArgs(material=Material(**shared, bump=bump2), transform=Matrix.translation(0, 1, 0)))])


def test_rtw_set_bump_limits_and_flatten_helpers():
    import raytracer_challenge_amd as rt
    hip = rt.hip_backend()
    assert hip.has_bump
    lib = hip.lib
    counts, desc = (C.c_uint32 * 8)(), ff.RtcSceneDesc()
    nw = hip.build_world(bumped_world())
    assert lib.rtw_world_flatten_counts(nw.handle, counts) == 0 and counts[5] == 1            # the two shapes share one material row
    e = lib.rtw_shape(0, (C.c_double * 16)(*Matrix.id().flat()), None, 1, None, 0)
    assert e
    assert lib.rtw_element_set_bump(None, RIPPLE, 0, 0.1, 1.0) != 0 and "NULL" in hip._err()
    for why, args in {"kind": (3, 0, 0.1, 1.0), "kind ": (-1, 0, 0.1, 1.0), "amplitude": (SIMPLEX, 0, math.nan, 1.0), "amplitude ": (RIPPLE, 0, math.inf, 1.0),
                      "frequency": (RIPPLE, 0, 0.1, 0.0), "frequency ": (SIMPLEX, 0, 0.1, math.nan), "octaves": (FRACTAL, 0, 0.1, 1.0),
                      "octaves ": (FRACTAL, MAX_OCTAVES + 1, 0.1, 1.0)}.items():
        assert lib.rtw_element_set_bump(e, *args) != 0 and "bump" in hip._err() and why.strip() in hip._err(), why
    assert lib.rtw_element_set_bump(e, FRACTAL, MAX_OCTAVES, 0.1, 1.0) == 0
    assert lib.rtw_element_set_bump(e, RIPPLE, 0, 0.0, 2.0) == 0                              # a second call replaces the first
    assert lib.rtw_world_add_element(nw.handle, e) == 0
    assert lib.rtw_world_flatten_counts(nw.handle, counts) != 0 and "bump" in hip._err()
    assert lib.rtw_world_flatten_desc(nw.handle, desc) != 0 and "bump" in hip._err()
    for world in (bumped_world(Bump.ripple(0.1, 1.0)), bumped_world(None, Bump.simplex(0.0, 1.0))):   # ... and through the Python layer
        nw2 = hip.build_world(world)
        assert lib.rtw_world_flatten_counts(nw2.handle, counts) != 0 and "bump" in hip._err()
    # a group takes the record for all its primitives; a material given to a group replaces its children's, bumps included
    kids = [Element.sphere(ShapeArgs(material=Material(bump=Bump.simplex(0.1, 1.0)))), Element.cube(ShapeArgs(transform=Matrix.translation(3, 0, 0)))]
    keeps = World([], [Element.composite(Matrix.id(), None, "aggregation", kids)])
    assert lib.rtw_world_flatten_counts(hip.build_world(keeps).handle, counts) != 0 and "bump" in hip._err()
    replaced = World([], [Element.composite(Matrix.id(), Material(diffuse=0.5), "aggregation", kids)])
    assert lib.rtw_world_flatten_counts(hip.build_world(replaced).handle, counts) == 0 and counts[5] == 1
    whole = World([], [Element.composite(Matrix.id(), Material(diffuse=0.5, bump=Bump.ripple(0.1, 2.0)), "aggregation", kids)])
    assert lib.rtw_world_flatten_counts(hip.build_world(whole).handle, counts) != 0 and "bump" in hip._err()


def test_exports_and_package_names():
    lib = load(LIB)
    for name in ("rtc_scene_create_ext4", "rtc_multi_create_ext4", "rtc_bump_normal", "rtc_bump_normals", "rtc_scene_bump_info", "rtw_element_set_bump"):
        assert hasattr(lib, name), name
    import raytracer_challenge_amd as rt
    from raytracer_challenge_amd import scenes
    assert rt.Bump is Bump
    cam, world = scenes.bump_showcase(32, 18)
    assert (cam.hsize, cam.vsize) == (32, 18) and world.background is not None and len(world.lights) == 1 and type(world.lights[0]).__name__ == "AreaLight"
    kinds = {}
    for e in world.elements:
        m = e.args.material if e.tag == "shape" else e.material
        kinds[m.bump.kind] = (e, m)
    assert set(kinds) == {"ripple", "fractal", "simplex"}
    floor, fm = kinds["ripple"]
    assert floor.geometry == "plane" and fm.reflective > 0 and fm.transparency == 0          # a rippled floor mirror
    ball, bm = kinds["fractal"]
    assert ball.geometry == "sphere" and bm.reflective > 0 and bm.transparency > 0 and bm.bump.octaves >= 2   # a fractal-bumped glass ball
    pot, _ = kinds["simplex"]
    assert pot.tag == "obj" and pot.path.endswith("teapot_low.obj") and " vn " in open(pot.path).read().replace("\nvn ", " vn ")   # smooth triangles
    hip = rt.hip_backend()
    nw = hip.build_world(world)
    assert nw.primitive_count > 200


def test_oracle_refuses_a_bump(orc):
    assert not orc.has_bump
    with pytest.raises(RtwError, match="a bump needs librtc_amd.so"):
        orc.build_world(bumped_world(Bump.ripple(0.1, 1.0)))
    with pytest.raises(RtwError, match="a bump needs librtc_amd.so"):
        orc.build_world(World([], [Element.composite(Matrix.id(), Material(bump=Bump.simplex(0.1, 1.0)), "aggregation", [Element.sphere()])]))
    orc.build_world(bumped_world())                                                            # no bump: as before


def test_emulator_refuses_a_bump():
    """tests/cpu_emu links the product's rtw_capi.cpp without rtc_scene_create_ext4 (the reference to it is weak): the library loads and
    renders worlds without a bump; a world with one fails with a message that names it."""
    from emu_lib import emu
    e = emu()
    cam = Camera.new(8, 6, 1.0, Camera.transform(Vector.point(0, 1.5, -5), Vector.point(0, 1, 0), Vector.vector(0, 1, 0)))
    rgb, _ = e.render(e.build_world(bumped_world()), cam, 1)
    assert np.isfinite(rgb).all() and rgb.max() > 0.0
    nw = e.build_world(bumped_world(Bump.ripple(0.1, 1.0)))
    with pytest.raises(RtwError, match="a bump .* needs rtc_scene_create_ext4"):
        e.render(nw, cam, 1)


def test_rust_shim_mirrors_rtc_bump():
    h = open(os.path.join(ROOT, "include", "rtc.h")).read()
    rs = open(os.path.join(ROOT, "shim", "gpu.rs")).read()
    c, r = c_struct(h, "rtc_bump"), rust_struct(rs, "RtcBump")
    assert c == r, (c, r)
    assert [f[0] for f in c] == [f[0] for f in RtcBump._fields_] and C.sizeof(RtcBump) == 32
    ci, ri = c_struct(h, "rtc_bump_info"), rust_struct(rs, "RtcBumpInfo")
    assert ci == ri, (ci, ri)
    assert [f[0] for f in ci] == [f[0] for f in RtcBumpInfo._fields_] and C.sizeof(RtcBumpInfo) == 32
    for fn in ("rtc_scene_create_ext4", "rtc_multi_create_ext4", "rtc_bump_normal", "rtc_bump_normals", "rtc_scene_bump_info"):
        assert "fn %s(" % fn in rs, fn
    assert "RTC_BUMP_SIMPLEX: i32 = 0" in rs and "RTC_BUMP_FRACTAL: i32 = 1" in rs and "RTC_BUMP_RIPPLE: i32 = 2" in rs
    assert "RTC_BUMP_SIMPLEX = 0, RTC_BUMP_FRACTAL = 1, RTC_BUMP_RIPPLE = 2" in h
    assert "RTC_BUMP_MAX_OCTAVES: u32 = %d" % MAX_OCTAVES in rs and "#define RTC_BUMP_MAX_OCTAVES %d" % MAX_OCTAVES in h


def test_the_bump_builds_are_extensions_of_the_general_rows_and_the_rule_is_one_function():
    """The NP instantiations of the one-kernel path are no rows of RTC_VARIANTS and have no table of their own (test_background_cpu.py holds
    the table and the Makefile's lists to that): they are extensions 2 (NP) and 3 (NP + BG) of the six general rows, rtc_bump.hip is built
    once, and the rule itself is one function."""
    import re
    csrc = os.path.join(ROOT, "raytracer_challenge_amd", "csrc")
    dev = open(os.path.join(csrc, "rtc_device.hpp")).read()
    assert re.findall(r"constexpr RtcVariant (\w+)\[", dev) == ["RTC_VARIANTS"]
    ext = dev[dev.index("enum RtcExt {"):]
    assert "RTC_EXT_NP = 2," in ext and "RTC_EXT_NP_BG = 3," in ext
    mk = open(os.path.join(csrc, "Makefile")).read()
    assert "VARIANT_IDS := 0 1 2 3 4 5 6 7 8 9 10 11\n" in mk and "GENERAL_IDS := 4 6 8 9 10 11\n" in mk and "EXT_IDS := 1 2 3\n" in mk
    small = re.search(r"^SMALL_UNITS := (.*)$", mk, re.M).group(1).split()
    assert small.count("rtc_bump") == 1 and "$(foreach u,$(SMALL_UNITS),$(O)/$(u).o): $(O)/%.o: %.hip $(SMALL_HDRS)\n\t$(HIPCC_C) -c $< -o $@\n" in mk
    assert "-ffp-contract=off" in mk and "bump_normal.h" in mk and "noise3.h" in mk
    khdrs = re.search(r"^KHDRS := (.*)$", mk, re.M).group(1).split()
    assert "bump_normal.h" in khdrs and "noise3.h" in khdrs and "SMALL_HDRS := $(KHDRS) " in mk   # every kernel object depends on them
    # the rule is one function: the kernels and the host entry call it, nothing restates it
    assert open(os.path.join(csrc, "bump_normal.h")).read().count("void rtc_bump_normal_at(") == 1
    for name in ("rtc_device.hpp", "rtc_bump.hip", "rtc_scene.cpp"):
        src = open(os.path.join(csrc, name)).read()
        assert "rtc_bump_normal_at(" in src, name
        assert "void rtc_bump_normal_at(" not in src, name   # called, not defined again
