"""The oracle's count of the de-duplicated ray tree (oracle/rt_oracle.hpp Counters::u_*, exported by orc_ray_counts and
orc_ray_counts_rays) held to (1) the reference recursion's own literal call counts through the L^d identity, (2) numbers written down by
hand, and then (3) the five ray counters the kernel source reports through the CPU emulator.  test_ray_counts_gpu.py holds the device's
rtc_stats to the same count."""
import math

import numpy as np
import pytest

import bump_cases as bc
import ext_cases as ec
import ray_counts as rc
from oracle_ext_lib import oracle_ext
from raytracer_challenge_amd.cabi import load
from raytracer_challenge_amd import scenes
from raytracer_challenge_amd.scene import (AreaLight, Background, Bump, Camera, Color, Element, Material, Matrix, Pattern, PointLight, ShapeArgs, SpotLight, Vector,
                                           World)

P, V = Vector.point, Vector.vector
WHITE = Color.new(1.0, 1.0, 1.0)


@pytest.fixture(scope="module")
def ext():
    return oracle_ext()


def by_depth(counts, key, n):
    return [int(x) for x in counts[key][:n]]


def nothing_beyond(counts, depth):
    return all(not counts[k][depth + 1:].any() for k in counts)


# ---- 1. the new count is the literal call count ----------------------------------------------------------------------------------------
def _lights(n):
    return [PointLight(Color.new(0.5, 0.5, 0.5), P(*p)) for p in ((-10.0, 10.0, -10.0), (8.0, 6.0, -4.0), (0.5, 9.0, 3.0))[:n]]


def _identity_cases():
    from test_fuzz_parity import random_case
    out = {"cover": lambda: scenes.cover(32, 32) + (5,),
           "glass_air_bubble": lambda: scenes.chapter11_glass_air_bubble(48, 24) + (5,)}
    for n in (2, 3):
        out["%d lights" % n] = (lambda n: lambda: (rc.two_light_glass_and_mirror()[0], World(_lights(n), rc.two_light_glass_and_mirror()[1].elements), 4))(n)
    for seed in (1000, 3001, 20002):
        out["fuzz %d" % seed] = (lambda s: lambda: (lambda c, w, f, _: (c, w, min(f, 4)))(*random_case(s, sizes=((32, 18),), counts=(17, 40))))(seed)
    return out


IDENTITY_CASES = _identity_cases()


@pytest.mark.parametrize("name", sorted(IDENTITY_CASES))
def test_unique_counts_times_L_to_the_d_are_the_literal_call_counts(orc, name):
    """The reference traces a subtree once per light (src/world.rs:58-79): a ray at depth d is traced L^d times.  The de-duplicated count
    is marked by Ctx::repeat == 0; the literal counts are the recursion's own.  (primary + reflect + refract)[d] * L^d == color_at[d] and
    shadow[d] * L^d == calls_shadow[d], exactly, and the grand total is orc_stats.unique_rays, which bench.py's CPU baseline reads."""
    cam, world, fuel = IDENTITY_CASES[name]()
    L = len(world.lights)
    assert L >= 1
    nw = orc.build_world(world)
    k = orc.ray_counts(nw, cam, fuel)
    assert nothing_beyond(k, fuel) and int(k["primary"][0]) == cam.hsize * cam.vsize and not k["primary"][1:].any()
    assert int(k["reflect"][0]) == 0 and int(k["refract"][0]) == 0 and int(k["container"][fuel]) == 0
    for d in range(fuel + 1):
        rays = int(k["primary"][d]) + int(k["reflect"][d]) + int(k["refract"][d])
        assert rays * L ** d == int(k["calls_color_at"][d]), (name, d)
        assert int(k["shadow"][d]) * L ** d == int(k["calls_shadow"][d]), (name, d)
    assert int(k["reflect"][1:].sum()) + int(k["refract"][1:].sum()) > 0, name   # (every case bounces)
    _, _, st = orc.render_timed(nw, cam, fuel)
    total = sum(int(k[c].sum()) for c in ("primary", "reflect", "refract", "shadow"))
    assert float(total) == st.unique_rays, (name, total, st.unique_rays)
    if L > 1:
        assert st.traced_rays > st.unique_rays


# ---- 2. scenes counted by hand ---------------------------------------------------------------------------------------------------------
def matte(**kw):
    return Material(pattern=Pattern.plain(Color.new(0.8, 0.7, 0.6)), specular=0.0, **kw)


def down_camera(w, h):
    return Camera.new(w, h, 0.8, Camera.transform(P(0.0, 5.0, 0.0), P(0.0, 0.0, 0.0), V(0.0, 0.0, 1.0)))


def rays_down(points, height=5.0):
    """Unit rays straight down onto (x, 0, z): the hit is (x, 0, z) and its over_point (x, 1e-5, z) without a rounding."""
    return np.array([(x, height, z, 0.0, -1.0, 0.0) for x, z in points], dtype=np.float64)


@pytest.mark.parametrize("L", [1, 3])
def test_a_matte_plane_sends_one_shadow_ray_per_light_and_hit(orc, ext, L):
    cam = down_camera(8, 6)
    world = World(_lights(L), [Element.plane(ShapeArgs(material=matte()))])
    for lib in (orc, ext):
        k = lib.ray_counts(lib.build_world(world), cam, 5)
        assert by_depth(k, "primary", 2) == [48, 0] and by_depth(k, "shadow", 2) == [L * 48, 0]          # every pixel looks at the plane
        assert k.totals() == {"rays_primary": 48, "rays_shadow": L * 48, "rays_reflect": 0, "rays_refract": 0, "rays_container": 0}
        assert by_depth(k, "calls_shadow", 1) == [L * 48]


@pytest.mark.parametrize("fuel", [0, 1, 4])
def test_a_mirror_corridor_reflects_every_ray_once_per_level(orc, fuel):
    """Two facing mirror planes (y = 0 and y = 2), the camera between them looking along z with an even number of rows (no ray is
    parallel to the planes): every ray hits a plane and leaves one reflected ray until the fuel is gone."""
    mirror = matte(reflective=0.5)
    world = World(_lights(1), [Element.plane(ShapeArgs(material=mirror)), Element.plane(ShapeArgs(transform=Matrix.translation(0.0, 2.0, 0.0), material=mirror))])
    cam = Camera.new(6, 4, 0.8, Camera.transform(P(0.0, 1.0, -3.0), P(0.0, 1.0, 0.0), V(0.0, 1.0, 0.0)))
    k = orc.ray_counts(orc.build_world(world), cam, fuel)
    assert by_depth(k, "primary", fuel + 2) == [24] + [0] * (fuel + 1)
    assert by_depth(k, "reflect", fuel + 2) == [0] + [24] * fuel + [0]
    assert by_depth(k, "shadow", fuel + 2) == [24] * (fuel + 1) + [0]
    assert not k["refract"].any() and not k["container"].any()


def glass_ball_world():
    """The book's chapter-11 worlds in one: a glass unit sphere (transparency 1, index 1.5) around an opaque sphere of radius 0.5."""
    glass = Material(pattern=Pattern.plain(Color.new(0.8, 1.0, 0.6)), diffuse=0.7, specular=0.2, transparency=1.0, refractive_index=1.5)
    return World([PointLight(WHITE, P(-10.0, 10.0, -10.0))], [Element.sphere(ShapeArgs(material=glass)), Element.sphere(ShapeArgs(transform=Matrix.scaling(0.5, 0.5, 0.5)))])


def test_total_internal_reflection_spawns_no_refracted_ray(orc, ext):
    """Chapter 11's rays.  From (0, 0, sqrt(2)/2) inside the glass along +y: the hit has n1 = 1.5, n2 = 1, cos_i = sqrt(2)/2, so
    sin2_t = 2.25 * 0.5 > 1 -- no refracted ray, but the hit's n1 / n2 were needed to decide that: container counts it.  From (0, 0, -5)
    along +z: one refracted ray at depth 1, which hits the opaque inner sphere."""
    tir = np.array([(0.0, 0.0, math.sqrt(2.0) / 2.0, 0.0, 1.0, 0.0)])
    through = np.array([(0.0, 0.0, -5.0, 0.0, 0.0, 1.0)])
    for lib in (orc, ext):
        nw = lib.build_world(glass_ball_world())
        k = lib.ray_counts_rays(nw, tir, 5)
        assert k.totals() == {"rays_primary": 1, "rays_shadow": 1, "rays_reflect": 0, "rays_refract": 0, "rays_container": 1}
        k = lib.ray_counts_rays(nw, through, 5)
        assert by_depth(k, "primary", 3) == [1, 0, 0] and by_depth(k, "refract", 3) == [0, 1, 0] and by_depth(k, "shadow", 3) == [1, 1, 0]
        assert by_depth(k, "container", 3) == [1, 0, 0] and not k["reflect"].any()
        both = lib.ray_counts_rays(nw, np.concatenate([tir, through, tir]), 5)
        assert both.totals() == {"rays_primary": 3, "rays_shadow": 4, "rays_reflect": 0, "rays_refract": 1, "rays_container": 3}


def test_fuel_zero_traces_the_primary_ray_and_its_shadow_rays_only(orc):
    """No fuel: no child ray, and n1 / n2 reach no result -- no container either."""
    nw = orc.build_world(glass_ball_world())
    k = orc.ray_counts_rays(nw, np.array([(0.0, 0.0, -5.0, 0.0, 0.0, 1.0), (0.0, 3.0, -5.0, 0.0, 0.0, 1.0)]), 0)     # the second ray hits nothing
    assert k.totals() == {"rays_primary": 2, "rays_shadow": 1, "rays_reflect": 0, "rays_refract": 0, "rays_container": 0}
    assert nothing_beyond(k, 0)


def test_a_reflective_weight_of_1e_300_spawns_a_ray_and_0_does_not(orc):
    """reflected_color tests `reflective == 0.0` (src/world.rs:90): the smallest weights still trace."""
    els = [Element.sphere(ShapeArgs(transform=Matrix.translation(-2.0, 0.0, 0.0), material=matte(reflective=0.0))),
           Element.sphere(ShapeArgs(transform=Matrix.translation(2.0, 0.0, 0.0), material=matte(reflective=1e-300))),
           Element.sphere(ShapeArgs(transform=Matrix.translation(6.0, 0.0, 0.0), material=matte(transparency=1e-300)))]
    nw = orc.build_world(World(_lights(1), els))
    at = lambda x: np.array([(x, 0.0, -5.0, 0.0, 0.0, 1.0)])  # noqa: E731
    assert orc.ray_counts_rays(nw, at(-2.0), 1).totals() == {"rays_primary": 1, "rays_shadow": 1, "rays_reflect": 0, "rays_refract": 0, "rays_container": 0}
    assert orc.ray_counts_rays(nw, at(2.0), 1).totals() == {"rays_primary": 1, "rays_shadow": 1, "rays_reflect": 1, "rays_refract": 0, "rays_container": 0}
    # straight through the centre of a transparent sphere of index 1: one refracted ray, which hits the far side (fuel 1: it ends there)
    assert orc.ray_counts_rays(nw, at(6.0), 1).totals() == {"rays_primary": 1, "rays_shadow": 2, "rays_reflect": 0, "rays_refract": 1, "rays_container": 1}


def test_a_4x4_area_light_sends_16_shadow_rays_per_hit(ext):
    cam = down_camera(8, 6)
    for jitter in (False, True):
        light = AreaLight(WHITE, P(-1.0, 4.0, -1.0), V(2.0, 0.0, 0.0), 4, V(0.0, 0.0, 2.0), 4, jitter=jitter)
        k = ext.ray_counts(ext.build_world(World([light], [Element.plane(ShapeArgs(material=matte()))])), cam, 5)
        assert k.totals() == {"rays_primary": 48, "rays_shadow": 16 * 48, "rays_reflect": 0, "rays_refract": 0, "rays_container": 0}


def test_a_hard_cone_sends_shadow_rays_to_the_lit_samples_only(ext):
    """include/rtc.h rtc_light_cone: a sample whose factor is 0.0 traces no shadow ray.  A hard-edged cone (inner == outer) over a matte
    plane, rays straight down at a grid of points: the expected number is the count of f != 0 from the product's own rtc_spot_factor at
    each over_point, which the oracle's restated factor must agree with."""
    import os
    from test_spot_lights_cpu import lib_spot_factor
    lib = load(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "raytracer_challenge_amd", "csrc", "librtc_amd.so"))
    origin, axis, angle = (0.5, 4.0, -0.25), (0.2, -1.0, 0.1), 0.4
    points = [(0.37 * i - 2.9, 0.41 * j - 2.7) for i in range(16) for j in range(14)]
    factors = []
    for x, z in points:
        code, f = lib_spot_factor(lib, axis, math.cos(angle), math.cos(angle), origin, (x, 1e-5, z))
        assert code == 0 and f in (0.0, 1.0)
        assert ext.spot_factor(axis, math.cos(angle), math.cos(angle), origin, (x, 1e-5, z)) == f
        factors.append(f)
    lit = sum(f != 0.0 for f in factors)
    assert 20 < lit < len(points) - 20
    world = World([SpotLight(WHITE, P(*origin), V(*axis), angle, angle), PointLight(Color.new(0.2, 0.2, 0.2), P(3.0, 6.0, 3.0))], [Element.plane(ShapeArgs(material=matte()))])
    k = ext.ray_counts_rays(ext.build_world(world), rays_down(points), 5)
    assert k.totals() == {"rays_primary": 224, "rays_shadow": lit + 224, "rays_reflect": 0, "rays_refract": 0, "rays_container": 0}


def test_a_miss_into_a_background_adds_nothing(ext):
    bg = Background(Pattern.plain(Color.new(0.2, 0.3, 0.9)))
    mirror = Element.plane(ShapeArgs(material=matte(reflective=0.5)))
    nw = ext.build_world(World(_lights(2), [mirror], bg))
    up = np.array([(0.0, 1.0, 0.0, 0.0, 1.0, 0.0)])                      # sees the background alone
    assert ext.ray_counts_rays(nw, up, 5).totals() == {"rays_primary": 1, "rays_shadow": 0, "rays_reflect": 0, "rays_refract": 0, "rays_container": 0}
    down = np.array([(0.0, 1.0, 0.0, 0.6, -0.8, 0.0)])                   # the plane, then its reflection into the background
    assert ext.ray_counts_rays(nw, down, 5).totals() == {"rays_primary": 1, "rays_shadow": 2, "rays_reflect": 1, "rays_refract": 0, "rays_container": 0}


# ---- 3. the two oracles, and bumps -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["glass_air_bubble", "nested_glass"])
def test_the_ext_oracle_counts_a_plain_world_as_the_plain_oracle_does(orc, ext, name):
    cam, world, fuel = rc.PLAIN_CASES[name]()
    a, b = orc.ray_counts(orc.build_world(world), cam, 3), ext.ray_counts(ext.build_world(world), cam, 3)
    assert set(a) == set(b) and all(np.array_equal(a[k], b[k]) for k in a)
    rays = np.array([(0.1 * i - 1.0, 1.0, -8.0, 0.01 * i, -0.1, 1.0) for i in range(24)])
    a, b = orc.ray_counts_rays(orc.build_world(world), rays, fuel), ext.ray_counts_rays(ext.build_world(world), rays, fuel)
    assert all(np.array_equal(a[k], b[k]) for k in a) and int(a["shadow"].sum()) > 0


def test_an_ext_world_with_more_than_one_light_is_counted_directly(ext):
    """An extension world evaluates the secondary colour once per hit, not once per light: the literal call counts are the unique counts
    themselves, and dividing them by L^d -- what orc_stats.unique_rays does -- would undercount."""
    cam, world = ec.everything_camera(13, 7), ec.everything_world(False)
    nw = ext.build_world(world)
    k = ext.ray_counts(nw, cam, 3)
    assert len(world.lights) == 3 and int(k["reflect"][2]) > 0
    assert np.array_equal(k["calls_shadow"], k["shadow"]) and np.array_equal(k["calls_color_at"], k["primary"] + k["reflect"] + k["refract"])
    _, _, st = ext.render_timed(nw, cam, 3)
    assert st.unique_rays < sum(int(k[c].sum()) for c in ("primary", "reflect", "refract", "shadow"))


def test_a_bump_changes_the_counts_only_where_the_shading_normal_decides(ext):
    """Total internal reflection is decided on the shading normal: the steep-bump scene traces other rays than its unbumped twin.  A record
    of amplitude 0 keeps the geometric normal's bits, and the twin's counts."""
    cam, world = ec.steep_camera(), ec.steep_world()
    twin = bc.bumped(world, lambda k: None)
    flat = bc.bumped(world, lambda k: (Bump.fractal(2, 0.0, 1.5), Bump.ripple(0.0, 0.9))[k % 2])
    counts = {name: ext.ray_counts(ext.build_world(w), cam, 4) for name, w in (("steep", world), ("twin", twin), ("flat", flat))}
    assert all(np.array_equal(counts["flat"][k], counts["twin"][k]) for k in counts["twin"])
    assert np.array_equal(counts["steep"]["primary"], counts["twin"]["primary"])
    assert int(counts["steep"]["container"][0]) == int(counts["twin"]["container"][0])        # the primary hits are the same
    assert not np.array_equal(counts["steep"]["refract"], counts["twin"]["refract"])
    assert not np.array_equal(counts["steep"]["shadow"], counts["twin"]["shadow"])


# ---- 4. the kernel source, through the CPU emulator ------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def emu():
    from emu_lib import emu as _emu
    return _emu()


_PLAIN_WANT = {}


def plain_want(orc, name):
    if name not in _PLAIN_WANT:
        cam, world, fuel = rc.PLAIN_CASES[name]()
        _PLAIN_WANT[name] = (cam, world, fuel, rc.expected(orc.ray_counts(orc.build_world(world), cam, fuel), cam.hsize * cam.vsize))
    return _PLAIN_WANT[name]


@pytest.mark.parametrize("path", ["1", "4"])
@pytest.mark.parametrize("name", sorted(rc.PLAIN_CASES))
def test_the_emulated_kernels_report_the_oracles_totals(emu, orc, name, path, monkeypatch):
    """rtc_stats as the kernel source fills it, both device paths, on the plain scenes of the GPU file: pixels and the five ray counters."""
    monkeypatch.setenv("RTC_KERNEL", path)
    cam, world, fuel, want = plain_want(orc, name)
    rc.assert_counts(rc.render_stats(emu, emu.build_world(world), cam, fuel), want, "%s path %s" % (name, path))


@pytest.mark.parametrize("path", ["1", "4"])
def test_the_emulated_kernels_by_depth_lists_ranges_and_rays(emu, orc, path, monkeypatch):
    """The differences between fuels are the oracle's depths; a sub-range, a pixel list with repeats and explicit rays count what the
    oracle counts over the same pixels and rays."""
    monkeypatch.setenv("RTC_KERNEL", path)
    cam, world = rc.two_light_glass_and_mirror()
    nw, nwo = emu.build_world(world), orc.build_world(world)
    n = cam.hsize * cam.vsize
    deep = orc.ray_counts(nwo, cam, 4)
    got = [rc.as_counts(rc.render_stats(emu, nw, cam, f)) for f in range(5)]
    rc.assert_counts(got[4], rc.expected(deep, n), "fuel 4")
    assert got[0]["rays_shadow"] == int(deep["shadow"][0]) and got[0]["rays_reflect"] == got[0]["rays_refract"] == got[0]["rays_container"] == 0
    for f in range(1, 5):
        for key in ("reflect", "refract", "shadow"):
            assert got[f]["rays_" + key] - got[f - 1]["rays_" + key] == int(deep[key][f]), (key, f)
        assert got[f]["rays_container"] - got[f - 1]["rays_container"] == int(deep["container"][f - 1]), f     # none at the last level
    first, m = 101, 333
    rc.assert_counts(rc.render_stats(emu, nw, cam, 3, first=first, n=m), rc.expected(orc.ray_counts(nwo, cam, 3, np.arange(first, first + m)), m), "sub-range")
    idx = np.random.default_rng(5).integers(0, n, 150).astype(np.uint64)
    idx[50:60] = idx[0]
    rc.assert_counts(rc.render_stats(emu, nw, cam, 3, pixel_indices=idx), rc.expected(orc.ray_counts(nwo, cam, 3, idx), len(idx)), "pixel list")
    rays = np.array([(0.2 * i - 2.0, 2.0, -6.0, 0.02 * i - 0.2, -0.25, 1.0) for i in range(70)])
    rc.assert_counts(rc.trace_stats(emu, nw, rays, 4), rc.expected(orc.ray_counts_rays(nwo, rays, 4), len(rays)), "explicit rays")
