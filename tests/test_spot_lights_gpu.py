"""Spot lights (include/rtc.h rtc_light_cone) on an MI355X, both device paths.  The oracle restates the reference, which has no cones,
so the device is pinned to it through equivalences the rule is built to have: an open cone is no cone, a dark cone is a light of
intensity 0, a hard edge partitions the frame into pixels of those two frames, a sample in the smooth band is a point light of
intensity I * f (f from rtc_spot_factor, itself pinned to a Python restatement by test_spot_lights_cpu.py), and a cone on an
unjittered area light is the same cone on its N sample points."""
import ctypes as C
import math

import numpy as np
import pytest

import foreign_flattener as ff
from foreign_flattener import render_scene
from raytracer_challenge_amd import scenes
from raytracer_challenge_amd.image import Image
from raytracer_challenge_amd.scene import (EPSILON, Adaptive, AreaLight, Camera, Color, Cone, Element, Filter, Material, Matrix, Pattern, PointLight, Sampling,
                                           ShapeArgs, SpotLight, Vector, World)
from test_area_lights_cpu import sample_positions
from test_spot_lights_cpu import (RtcLightCone, cone_c, lib_spot_factor, partition_classes, partition_fixture, partition_lights)

pytestmark = pytest.mark.gpu
PATHS = ["1", "4"]
vp = C.c_void_p
DOWN = Vector.vector(0.0, -1.0, 0.0)


def render_world(hip, world, cam, fuel):
    """The same through the Python layer: SpotLight / AreaLight(cone=) -> rtw -> rtc_scene_create_ext2."""
    lib = hip.lib
    nw = hip.build_world(world)
    scene = lib.rtw_world_scene(nw.handle, 0)
    assert scene, hip._err()
    out = render_scene(lib, scene, cam, fuel)
    nw.close()
    return out


def same_frames(a, b, what, shadow=True):
    assert np.array_equal(a[0].view(np.uint64), b[0].view(np.uint64)), "%s: pixels differ" % what
    assert a[1].tobytes() == b[1].tobytes(), "%s: primary hit records differ" % what
    assert np.array_equal(a[2], b[2]), "%s: hit-tree digests differ" % what
    if shadow:
        assert a[3].rays_shadow == b[3].rays_shadow, "%s: rays_shadow %d != %d" % (what, a[3].rays_shadow, b[3].rays_shadow)


def with_cones(world, inner, outer, axis=DOWN, only=None):
    """Every light of the world (or light `only`) with the cone (axis, inner, outer); area lights keep their samples."""
    out = []
    for i, l in enumerate(world.lights):
        if only is not None and i != only:
            out.append(l)
        elif isinstance(l, AreaLight):
            out.append(AreaLight(l.intensity, l.corner, l.uvec, l.usteps, l.vvec, l.vsteps, l.jitter, cone=Cone(axis, inner, outer)))
        else:
            out.append(SpotLight(l.intensity, l.origin, axis, inner, outer))
    return World(out, world.elements)


def as_area(world, n, jitter):
    """Each point light as an n x n area light of 1 x 1 units centred on it (in the xz plane)."""
    P, V = Vector.point, Vector.vector
    return World([AreaLight(l.intensity, P(l.origin[0] - 0.5, l.origin[1], l.origin[2] - 0.5), V(1.0, 0.0, 0.0), n, V(0.0, 0.0, 1.0), n, jitter)
                  for l in world.lights], world.elements)


def small_scenes():
    return (("cover",) + scenes.cover(24, 16), ("glass_air_bubble",) + scenes.chapter11_glass_air_bubble(19, 11))


# ---- 1. an open cone is no cone, at every depth ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("path", PATHS)
def test_open_cone_is_no_cone(hip, path, monkeypatch):
    monkeypatch.setenv("RTC_KERNEL", path)
    for name, cam, world in small_scenes():
        for kind, w in (("point", world), ("area 2x2", as_area(world, 2, False)), ("area 3x3 jittered", as_area(world, 3, True))):
            plain = render_world(hip, w, cam, 5)
            opened = render_world(hip, with_cones(w, math.pi, math.pi), cam, 5)     # cos_inner = cos_outer = cos(pi) = -1.0
            assert Cone(DOWN, math.pi, math.pi).cos_inner == -1.0
            same_frames(opened, plain, "%s %s path %s" % (name, kind, path))
            assert plain[3].rays_shadow > 0 and np.isfinite(plain[0]).all() and plain[0].max() > 0.0


# ---- 2. a dark cone is a light of intensity 0 -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("path", PATHS)
def test_dark_cone_is_a_light_of_intensity_zero(hip, path, monkeypatch):
    monkeypatch.setenv("RTC_KERNEL", path)
    # every scene lies below and in front of its lights' +y: an axis straight up with cos_inner = cos_outer = 1 points away from all of it
    up = Vector.vector(0.0, 1.0, 0.0)
    for name, cam, world in small_scenes():
        if len(world.lights) == 1:   # (a second light keeps the frame from being black)
            world = World(world.lights + [PointLight(Color(0.3, 0.3, 0.4), Vector.point(-5.0, 8.0, 3.0))], world.elements)
        for which in range(len(world.lights)):
            dark = render_world(hip, with_cones(world, 0.0, 0.0, axis=up, only=which), cam, 5)
            zero = render_world(hip, World([PointLight(Color(0.0, 0.0, 0.0), l.origin) if i == which else l for i, l in enumerate(world.lights)], world.elements), cam, 5)
            plain = render_world(hip, world, cam, 5)
            same_frames(dark, zero, "%s light %d path %s" % (name, which, path), shadow=False)
            assert zero[3].rays_shadow == plain[3].rays_shadow and zero[3].rays_shadow % len(world.lights) == 0
            per_light = zero[3].rays_shadow // len(world.lights)          # every hit sends one shadow ray per light
            assert per_light > 0 and dark[3].rays_shadow == zero[3].rays_shadow - per_light, (name, which, dark[3].rays_shadow, zero[3].rays_shadow)
            assert not np.array_equal(dark[0], plain[0])                   # ... and the light did matter


# ---- 3. a hard edge partitions the frame -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("path", PATHS)
def test_hard_edge_partitions_the_frame(hip, orc, path, monkeypatch):
    monkeypatch.setenv("RTC_KERNEL", path)
    spot, plain, zero = partition_lights()
    cam, _ = partition_fixture(plain)
    frames = {k: render_world(hip, partition_fixture(l)[1], cam, 0) for k, l in (("spot", spot), ("plain", plain), ("zero", zero))}
    _, ref_hits = orc.render(orc.build_world(partition_fixture(plain)[1]), cam, 0)
    assert frames["spot"][1].tobytes() == ref_hits.tobytes()
    rays = hip.camera_rays(cam, Sampling()).reshape(-1, 6)
    c, lit, dark, excluded = partition_classes(rays, ref_hits)
    n = float(len(c))
    assert lit.sum() >= 0.15 * n and dark.sum() >= 0.15 * n and excluded.sum() <= 0.02 * n
    px = {k: v[0].view(np.uint64) for k, v in frames.items()}
    is_plain, is_zero = (px["spot"] == px["plain"]).all(axis=1), (px["spot"] == px["zero"]).all(axis=1)
    assert (is_plain | is_zero).all(), "%d pixels are neither the cone-less frame's nor the intensity-0 frame's" % int((~(is_plain | is_zero)).sum())
    assert is_plain[lit].all() and not is_zero[lit].any(), "lit pixels: %d differ from the cone-less frame" % int((~is_plain[lit]).sum())
    assert is_zero[dark].all() and not is_plain[dark].any(), "dark pixels: %d differ from the intensity-0 frame" % int((~is_zero[dark]).sum())
    assert frames["spot"][3].rays_shadow == int(lit.sum()) + int((is_plain & excluded).sum())   # no shadow ray outside the cone
    print("path %s: %d lit, %d dark, %d excluded pixels" % (path, lit.sum(), dark.sum(), excluded.sum()))


# ---- 4. the smooth band against the oracle, ray by ray ----------------------------------------------------------------------------------
@pytest.mark.parametrize("path", PATHS)
def test_smooth_band_against_the_oracle_ray_by_ray(hip, orc, path, monkeypatch):
    monkeypatch.setenv("RTC_KERNEL", path)
    lib = hip.lib
    mat = Material(pattern=Pattern.plain(Color(0.9, 0.8, 0.7)), ambient=0.1, diffuse=0.8, specular=0.0)
    els = [Element.plane(ShapeArgs(material=mat)), Element.sphere(ShapeArgs(transform=Matrix.translation(0.9, 1.5, 0.3) * Matrix.scaling(0.4, 0.4, 0.4)))]
    inten, pos, axis = Color(1.0, 0.9, 0.8), Vector.point(0.5, 4.0, -0.25), Vector.vector(0.2, -2.0, 0.1)
    inner, outer = 0.3, 0.6
    spot = SpotLight(inten, pos, axis, inner, outer)
    rng = np.random.default_rng(31)
    # hit points spread over a disc that reaches beyond the outer cone (radius 4 tan(0.6) = 2.7)
    r, phi = 3.6 * np.sqrt(rng.uniform(0.0, 1.0, 64)), rng.uniform(0.0, 2.0 * math.pi, 64)
    target = np.column_stack([0.5 + r * np.cos(phi), np.zeros(64), -0.25 + r * np.sin(phi)])
    o = np.column_stack([rng.uniform(-2, 2, 64), np.full(64, 3.0), rng.uniform(-2, 2, 64)])
    d = target - o
    d /= np.sqrt((d * d).sum(1))[:, None]
    rays = np.hstack([o, d])
    rgb, hits = hip.color_at(hip.build_world(World([spot], els)), rays, 0)
    _, ref_hits = orc.color_at(orc.build_world(World([PointLight(inten, pos)], els)), rays, 0)
    assert hits.tobytes() == ref_hits.tobytes()
    on_floor = np.flatnonzero(hits["prim"] == 0)
    assert on_floor.size >= 56
    counts = {"inner": 0, "band": 0, "outside": 0}
    for i in on_floor:
        over = (o[i] + d[i] * hits["t"][i]) + np.array([0.0, 1.0, 0.0]) * EPSILON      # src/ray.rs:10-12, src/intersection.rs:54-65
        rc, f = lib_spot_factor(lib, axis, spot.cone.cos_inner, spot.cone.cos_outer, pos, over)
        assert rc == 0
        counts["inner" if f == 1.0 else "outside" if f == 0.0 else "band"] += 1
        scaled = PointLight(Color(inten.r * f, inten.g * f, inten.b * f), pos)          # one multiplication per channel
        want, _ = orc.color_at(orc.build_world(World([scaled], els)), rays[i:i + 1], 0)
        assert np.array_equal(rgb[i].view(np.uint64), want[0].view(np.uint64)), "ray %d (f = %r): device %s, oracle %s" % (i, f, rgb[i], want[0])
    print("path %s: %s" % (path, counts))
    assert counts["band"] >= 16 and counts["inner"] >= 4 and counts["outside"] >= 4, counts


# ---- 5. area x cone -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("path", PATHS)
def test_cone_on_an_area_light_is_the_cone_on_its_sample_points(hip, path, monkeypatch):
    monkeypatch.setenv("RTC_KERNEL", path)
    cam, world = partition_fixture(partition_lights()[1])
    cone = Cone(Vector.vector(0.3, -1.0, 0.1), 0.35, 0.6)
    area = AreaLight(Color(1.0, 0.9, 0.8), Vector.point(-0.5, 5.0, -0.75), Vector.vector(1.0, 0.0, 0.0), 2, Vector.vector(0.0, 0.0, 1.5), 3, cone=cone)
    n = float(area.samples)
    sixth = Color(area.intensity.r / n, area.intensity.g / n, area.intensity.b / n)
    spots = [SpotLight(sixth, Vector.point(*p), cone.direction, cone.inner_angle, cone.outer_angle) for p in sample_positions(area)]
    assert len(spots) == 6
    a = render_world(hip, World([area], world.elements), cam, 0)
    b = render_world(hip, World(spots, world.elements), cam, 0)
    same_frames(a, b, "2x3 area light with a cone, path %s" % path)
    lit = (a[0] != 0.0).any(axis=1)
    assert 0.1 < lit.mean() < 0.9                                                       # the cone cuts the frame
    no_cone = render_world(hip, World([AreaLight(area.intensity, area.corner, area.uvec, 2, area.vvec, 3)], world.elements), cam, 0)
    band = lit & (a[0] != no_cone[0]).any(axis=1)
    assert band.sum() >= 16 and a[3].rays_shadow < no_cone[3].rays_shadow               # a smooth edge, and fewer shadow rays


# ---- 6. plumbing ----------------------------------------------------------------------------------------------------------------------------
def spot_world():
    cam, world = partition_fixture(partition_lights()[1])
    lights = [SpotLight(Color(1.0, 0.9, 0.8), Vector.point(0.0, 5.0, 0.0), Vector.vector(0.1, -1.0, 0.05), 0.4, 0.6),
              PointLight(Color(0.2, 0.2, 0.3), Vector.point(-6.0, 7.0, -4.0))]
    return cam, World(lights, world.elements)


@pytest.mark.parametrize("path", PATHS)
def test_create_ext2_multi_and_zero_cones(hip, path, monkeypatch):
    monkeypatch.setenv("RTC_KERNEL", path)
    lib = hip.lib
    cam, world = spot_world()
    want = render_world(hip, world, cam, 5)
    flat = ff.flatten(World([PointLight(l.intensity, l.origin) for l in world.lights], world.elements))
    desc = flat.desc()
    c = world.lights[0].cone
    cones = (RtcLightCone * 1)(cone_c(0, c.direction, c.cos_inner, c.cos_outer))
    s = vp()
    assert lib.rtc_scene_create_ext2(C.byref(desc), None, cones, 1, 0, C.byref(s)) == 0, lib.rtc_last_error()
    got = render_scene(lib, s, cam, 5)
    lib.rtc_scene_destroy(s)
    same_frames(got, want, "cones on desc->lights, path %s" % path)
    # one device listed twice
    m, devs = vp(), (C.c_int * 2)(0, 0)
    assert lib.rtc_multi_create_ext2(C.byref(desc), None, cones, 1, devs, 2, C.byref(m)) == 0, lib.rtc_last_error()
    rc, mrgb = ff.make_camera(cam), np.full((cam.hsize * cam.vsize, 3), np.nan)
    assert lib.rtc_render_multi(m, C.byref(rc), 5, mrgb.ctypes.data, None) == 0, lib.rtc_last_error()
    lib.rtc_multi_destroy(m)
    assert np.array_equal(mrgb.view(np.uint64), want[0].view(np.uint64))
    # zero cones: rtc_scene_create_ext
    a, b = vp(), vp()
    assert lib.rtc_scene_create_ext2(C.byref(desc), None, None, 0, 0, C.byref(a)) == 0, lib.rtc_last_error()
    assert lib.rtc_scene_create_ext(C.byref(desc), None, 0, C.byref(b)) == 0, lib.rtc_last_error()
    ra, rb = render_scene(lib, a, cam, 5), render_scene(lib, b, cam, 5)
    lib.rtc_scene_destroy(a)
    lib.rtc_scene_destroy(b)
    same_frames(ra, rb, "zero cones, path %s" % path)
    assert not np.array_equal(ra[0], want[0])


@pytest.mark.parametrize("path", PATHS)
def test_sampled_filtered_and_adaptive_cameras_take_spot_scenes(hip, path, monkeypatch):
    monkeypatch.setenv("RTC_KERNEL", path)
    cam, world = spot_world()
    nw = hip.build_world(world)
    sp = Sampling(2)
    got = hip.render_sampled(nw, cam, sp, 0)
    rays = hip.camera_rays(cam, sp)                                         # [n, 4, 6]
    col, _ = hip.color_at(nw, rays.reshape(-1, 6), 0)
    col = col.reshape(-1, 4, 3)
    mean = (((col[:, 0] + col[:, 1]) + col[:, 2]) + col[:, 3]) / 4.0
    assert np.array_equal(got.view(np.uint64), mean.view(np.uint64))
    assert np.array_equal(hip.render_filtered(nw, cam, sp, Filter.box(0.5), 0), got)
    assert np.array_equal(hip.render_adaptive(nw, cam, Adaptive(Sampling(), sp, math.inf), 0), hip.render(nw, cam, 0, want_hits=False)[0])


@pytest.mark.parametrize("path", PATHS)
def test_uv_scene_with_a_spot(hip, path, monkeypatch):
    monkeypatch.setenv("RTC_KERNEL", path)
    cam, world = scenes.texture_showcase(40, 24)
    plain = render_world(hip, world, cam, 3)
    opened = render_world(hip, with_cones(world, math.pi, math.pi), cam, 3)
    same_frames(opened, plain, "texture_showcase, open cone, path %s" % path)
    cone = render_world(hip, with_cones(world, 0.08, 0.2, axis=Vector.vector(8.0, -9.0, 10.5)), cam, 3)
    assert cone[1].tobytes() == plain[1].tobytes() and np.array_equal(cone[2], plain[2])       # the same hits, another light
    assert not np.array_equal(cone[0], plain[0]) and cone[3].rays_shadow < plain[3].rays_shadow
    monkeypatch.setenv("RTC_KERNEL", "4" if path == "1" else "1")                              # ... and the other path's bits
    other = render_world(hip, with_cones(world, 0.08, 0.2, axis=Vector.vector(8.0, -9.0, 10.5)), cam, 3)
    same_frames(cone, other, "texture_showcase with a spot, both paths")


def test_par_render_of_spot_showcase(hip, monkeypatch):
    cam, world = scenes.spot_showcase(96, 54)
    img = Image.par_render(cam, world)
    px = np.asarray(img.pixels).reshape(-1, 3)
    assert px.shape == (96 * 54, 3) and np.isfinite(px).all() and px.max() > 0.2
    frames = []
    for path in PATHS:
        monkeypatch.setenv("RTC_KERNEL", path)
        frames.append(render_world(hip, world, cam, 5))
    same_frames(frames[0], frames[1], "spot_showcase, both paths")
    assert np.array_equal(frames[0][0], px)
