"""Bilinear image-texture lookups (include/rtc.h RTC_UV_IMAGE_LINEAR*) on an MI355X, both device paths.  The oracles know no such rule, so
the device is held to rtc_texture_sample -- the host build of the function the kernels compile, itself pinned to a Python restatement by
test_texture_filter_cpu.py -- and to identities against frames the oracles do hold: a 2x1 texture is a Gradient, a one-colour texture is
Plain, a clamped axis at an integer is the nearest texel."""
import ctypes as C
import math

import numpy as np
import pytest

import build_matrix as bm
import foreign_flattener as ff
from raytracer_challenge_amd import Texture, UvPattern, scenes
from raytracer_challenge_amd.device import RtcStatsC
from raytracer_challenge_amd.image import Image
from raytracer_challenge_amd.scene import (AreaLight, Background, Color, Element, Material, Matrix, Pattern, PointLight, Sampling, ShapeArgs, Vector,
                                           World)
from test_background_cpu import BG_CUBE, background_points
from test_background_gpu import background_colors, render_world
from test_sampled_camera_gpu import sampled
from test_texture_filter_cpu import (LINEAR, LINEAR_KINDS, LINEAR_WRAP, LINEAR_WRAP_U, NEAREST, SIZES, SURFACES, SURFACE_FRAME, HostTexture, floor_ties, linear, seeded, uv_set)
from test_texture_map_cpu import near_threshold, uv_map
from test_texture_map_gpu import (CASES, MAPS, T_PATTERN, RtcSceneExt, UvFlat, cam, flat_world, mapped, points, seeded_texture, shading_world)
from wf_level_classes import trace_rays

pytestmark = pytest.mark.gpu
PATHS = ["1", "4"]
vp = C.c_void_p
LIGHT = [PointLight(Color.white(), Vector.point(-10, 10, -10))]


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def host_colours(lib, face, uv):
    """rtc_texture_sample of a UvPattern image record at each (u, v)."""
    t = HostTexture(lib, face.texture.rgb)
    code = face.kind_code()
    return np.array([t.sample(code, float(u), float(v)) for u, v in uv])


def identity_point(d):
    """The root node's transform_inv, the identity, on the point (dx, dy, dz, 1.0): its four terms in the device's order (0 * inf is NaN, so
    an infinite component poisons the others)."""
    x, y, z = (np.float64(c) for c in d)
    one, zero = np.float64(1.0), np.float64(0.0)
    with np.errstate(all="ignore"):
        return (float(one * x + zero * y + zero * z + zero * one), float(zero * x + one * y + zero * z + zero * one),
                float(zero * x + zero * y + one * z + zero * one))


# ---- 1. device against host, no tracing ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size", SIZES, ids=lambda s: "%dx%d" % s)
def test_background_lookups_are_rtc_texture_sample(hip, size):
    """A background that is a planar-mapped image under RTC_BG_DIRECTION: the point is the direction given, so (dx, ., dz) looks up
    (m1(dx), m1(dz)) -- rtc_background_colors evaluates the pattern tree on the device with no ray traced."""
    w, h = size
    tex = Texture(seeded(w, h))
    pts = uv_set(w, h)
    dirs = np.array([(u, 0.3, v) for u, v in pts])
    uv = []
    for d in dirs:
        _, u, v = uv_map(MAPS["planar"], *identity_point(d))
        uv.append((u, v))
    for kind in LINEAR_KINDS:
        face = linear(tex, kind)
        world = World(LIGHT, [Element.sphere(ShapeArgs())], Background(Pattern.texture_map(Matrix.id(), "planar", face), "direction"))
        nw = hip.build_world(world)
        got = background_colors(hip, nw, dirs)
        nw.close()
        want = host_colours(hip.lib, face, uv)
        bad = np.flatnonzero((bits(got) != bits(want)).any(axis=1))
        assert bad.size == 0, "%dx%d kind %d: %d of %d lookups differ, first (u, v) %s: device %s host %s" % (
            w, h, kind, bad.size, len(pts), pts[bad[0]], got[bad[0]], want[bad[0]])


def test_skybox_faces_and_seams_are_rtc_texture_sample(hip):
    """RTC_BG_CUBE with six different clamped linear textures: every face, and directions on the seams between faces (two or three
    components of equal magnitude: the cube map's first matching test decides, and u or v is exactly 0 or 1 there)."""
    sizes = [(5, 3), (9, 5), (37, 23), (2, 2), (1, 4), (4, 1)]
    faces = [linear(Texture(seeded(w, h, seed=50 + k)), LINEAR) for k, (w, h) in enumerate(sizes)]
    rng = np.random.default_rng(17)
    dirs = [rng.normal(size=3) * rng.choice([1.0, 1e-3, 40.0]) for _ in range(3000)]
    for a in (1.0, -1.0):
        for b in (1.0, -1.0):
            for c in (0.3, -0.7, 1.0, -1.0, 0.0):
                dirs += [(a, b, c), (a, c, b), (c, a, b), (2.5 * a, 2.5 * b, 2.5 * c), (0.1 * a, 0.1 * c, 0.1 * b)]
    dirs += [(1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1)]
    dirs = np.array(dirs, dtype=np.float64)
    world = World(LIGHT, [Element.sphere(ShapeArgs())], Background(Pattern.cube_map(Matrix.id(), *faces), "cube"))
    nw = hip.build_world(world)
    got = background_colors(hip, nw, dirs)
    nw.close()
    p = background_points(BG_CUBE, dirs)
    seen = set()
    want = np.empty_like(got)
    samplers = [HostTexture(hip.lib, f.texture.rgb) for f in faces]
    for i, q in enumerate(p):
        face, u, v = uv_map(MAPS["cube"], *identity_point(q))
        seen.add(face)
        want[i] = samplers[face].sample(LINEAR, u, v)
    assert seen == set(range(6))
    bad = np.flatnonzero((bits(got) != bits(want)).any(axis=1))
    assert bad.size == 0, "%d of %d directions differ, first %s: device %s host %s" % (bad.size, len(dirs), dirs[bad[0]], got[bad[0]], want[bad[0]])


# ---- 2. pattern space on surfaces ---------------------------------------------------------------------------------------------------
# The planar and cube maps are f64 +, -, *, / and floor: the device's (u, v) is the restatement's, bit for bit.  The spherical and
# cylindrical maps go through atan2 (and acos), where the device's maths library and the C library behind the restatement are two
# implementations, each within its own error of the true value: OpenCL's full-profile bounds for f64 (atan2 6 ulp, acos 4 ulp; the
# device library documents less) plus the C library's 1 ulp put theta within 7 ulp(pi) = 7 * 2^-51 and phi within 5 * 2^-51.  In units
# of 2^-53, the grid u = 1 - (theta / 2 pi + 0.5) and v = 1 - phi / pi live on near 1: 7 * 4 / (2 pi) = 4.5 and 5 * 4 / pi = 6.4, and
# the two roundings that follow add one unit each.  The lookup is continuous in (u, v), so an ulp of u moves the colour by an ulp-sized
# amount instead of leaving the texel where it was: there the device's colour must be, bit for bit, rtc_texture_sample at SOME (u', v')
# of that window around the restated (u, v) -- still exact in the lookup rule, and no wider than the maps' own uncertainty.
U_WINDOW, V_WINDOW = 6, 8          # units of 2^-53
GRID = 2.0 ** -53


def window_match(sampler, kind, u, v, got, du, dv):
    for i in sorted(range(-du, du + 1), key=abs):
        for j in sorted(range(-dv, dv + 1), key=abs):
            if bits(np.array(sampler.sample(kind, u + i * GRID, v + j * GRID))).tolist() == bits(got).tolist():
                return True
    return False


@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("surface", range(len(SURFACES)))
def test_linear_render_is_rtc_texture_sample_at_the_pattern_space_point(hip, orc, path, surface, monkeypatch):
    """A Checkers(T, Debug, Debug) render, pinned to the oracle, gives the point a UV node with transform T sees; with ambient 1 and
    nothing else a pixel is its pattern colour: the host's sample at the restated map of that point -- for the planar and the cube map
    at exactly the restated (u, v); for the spherical and the cylindrical map within the few units of 2^-53 by which two atan2 / acos may
    differ (above).  Measured on an MI355X, 64x48, either path: spherical 22 of 206 and cylindrical 38 of 308 hit pixels differ from the sample
    at the C library's own (u, v), by at most 5.1e-15 and 6.9e-15; every one of them is the sample at a neighbouring (u', v'); planar (2880
    pixels) and cube (391) are the sample at the restated (u, v) itself."""
    monkeypatch.setenv("RTC_KERNEL", path)
    case, kind = SURFACES[surface]
    shape, transform, mapping = CASES[case]
    c = cam(*SURFACE_FRAME)
    pts, hit = points(hip, orc, shape, transform, T_PATTERN, c, path)
    faces = [linear(seeded_texture(11 + k), kind) for k in range(6 if mapping == "cube" else 1)]
    rgb, _ = hip.render(hip.build_world(flat_world(shape, transform, mapped(mapping, faces))), c, 5)
    samplers = [HostTexture(hip.lib, f.texture.rgb) for f in faces]
    want = np.zeros_like(pts)
    tie = np.zeros(len(pts), dtype=bool)
    uvs = {}
    for i in np.flatnonzero(hit):
        face, u, v = uv_map(MAPS[mapping], *pts[i])
        uvs[i] = (face, u, v)
        want[i] = samplers[face].sample(kind, u, v)
        tie[i] = floor_ties(faces[face], u, v) or (mapping in ("spherical", "cylindrical") and abs(pts[i][0]) < 1e-9 and pts[i][2] < 0.0)
    use = hit & ~tie
    n_tie = int((hit & tie).sum())
    bad = use & (bits(rgb) != bits(want)).any(axis=1)
    print("%s kind %d (RTC_KERNEL=%s): %d hit pixels, %d excluded as threshold ties, %d differ at the restated (u, v), max |d| %.3e" % (
        mapping, kind, path, int(hit.sum()), n_tie, int(bad.sum()), float(np.abs(rgb - want)[use].max()) if use.any() else 0.0))
    assert hit.sum() > 150 and n_tie <= 0.01 * hit.sum(), (mapping, int(hit.sum()), n_tie)
    if mapping in ("spherical", "cylindrical"):
        dv = V_WINDOW if mapping == "spherical" else 0       # the cylindrical v is m1(y): exact
        for i in np.flatnonzero(bad):
            face, u, v = uvs[i]
            if window_match(samplers[face], kind, u, v, rgb[i], U_WINDOW, dv):
                bad[i] = False
        print("  %d differ from every sample of the window" % int(bad.sum()))
    assert not bad.any(), "%s: %d pixels differ from rtc_texture_sample, first %s: got %s want %s" % (
        mapping, int(bad.sum()), np.flatnonzero(bad)[:3], rgb[bad][:3], want[bad][:3])


# ---- 3. identities on full ray trees ------------------------------------------------------------------------------------------------
LIGHTS = [PointLight(Color(0.8, 0.8, 0.8), Vector.point(-6, 8, -6)),
          AreaLight(Color(0.4, 0.4, 0.5), Vector.point(3, 6, -4), Vector.vector(1.5, 0, 0), 2, Vector.vector(0, 0, 1.5), 2, True)]
C0, C1 = (0.25, 0.5, 0.75), (0.75, 0.25, 0.5)      # dyadic: c0 + (c1 - c0) * 1.0 is exactly c1


def tree_cam():
    return cam(64, 48, frm=(0.0, 3.5, -7.0), to=(0.0, 0.8, 0.5))


def same_render(a, b, what):
    assert np.array_equal(bits(a[0]), bits(b[0])), "%s: %d pixels differ" % (what, int((bits(a[0]) != bits(b[0])).any(axis=1).sum()))
    assert a[1].tobytes() == b[1].tobytes(), "%s: primary hit records differ" % what
    assert np.array_equal(a[2], b[2]), "%s: hit-tree digests differ" % what
    for k in ("rays_primary", "rays_shadow", "rays_reflect", "rays_refract", "rays_container"):
        assert getattr(a[3], k) == getattr(b[3], k), "%s: %s" % (what, k)


@pytest.mark.parametrize("path", PATHS)
def test_two_texels_are_a_gradient(hip, path, monkeypatch):
    """2x1 {c0, c1}, both axes clamped, planar: x = u * 1.0 = m1(px), the Gradient's frac, and the colour is its lerp.  The Gradient
    render is held to the reference oracle by the existing suites, so this holds the new path's full ray tree to the reference."""
    monkeypatch.setenv("RTC_KERNEL", path)
    tex = Texture(np.array([[C0, C1]]))
    uvp = Pattern.texture_map(T_PATTERN, "planar", linear(tex, LINEAR))
    grad = Pattern.gradient(T_PATTERN, Pattern.plain(Color(*C0)), Pattern.plain(Color(*C1)))
    a = render_world(hip, World(LIGHTS, shading_world(lambda k: uvp)), tree_cam())
    b = render_world(hip, World(LIGHTS, shading_world(lambda k: grad)), tree_cam())
    assert a[3].rays_reflect > 0 and a[3].rays_refract > 0 and len(np.unique(bits(b[0]))) > 500
    same_render(a, b, "2x1 linear texture against the gradient (RTC_KERNEL=%s)" % path)


@pytest.mark.parametrize("path", PATHS)
def test_one_colour_textures_shade_like_plain(hip, path, monkeypatch):
    monkeypatch.setenv("RTC_KERNEL", path)
    c = (0.7, 0.45, 0.2)
    tex = Texture(np.broadcast_to(np.array(c), (3, 5, 3)))
    b = render_world(hip, World(LIGHTS, shading_world(lambda k: Pattern.plain(Color(*c)))), tree_cam())
    for kind in LINEAR_KINDS:
        face = linear(tex, kind)

        def pattern_for(shape):
            mapping = {"sphere": "spherical", "cylinder": "cylindrical", "cube": "cube"}.get(shape, "planar")
            return mapped(mapping, [face] * 6)
        a = render_world(hip, World(LIGHTS, shading_world(pattern_for)), tree_cam())
        same_render(a, b, "one-colour 5x3 texture of kind %d against Plain (RTC_KERNEL=%s)" % (kind, path))


@pytest.mark.parametrize("path", PATHS)
def test_texel_centres_of_a_clamped_axis_are_the_nearest_texels(hip, path, monkeypatch):
    """9x5 under an untransformed planar map on the floor: rays straight down onto (i/8, 0, 1 - j/4) land at u = i/8, v = 1 - j/4, where x
    is the integer i (and j for the rows) and t is 0: kind 3 gives kind 2's colours bit for bit, and both are the texel's."""
    tex = Texture(seeded(9, 5))
    rays = np.array([(i / 8.0, 5.0, 1.0 - j / 4.0, 0.0, -1.0, 0.0) for j in range(1, 5) for i in range(8)])
    out = {}
    for kind, face in ((NEAREST, UvPattern.image(tex)), (LINEAR, linear(tex, LINEAR))):
        world = flat_world("plane", Matrix.id(), Pattern.texture_map(Matrix.id(), "planar", face))
        out[kind] = trace_rays(hip, world, rays, 5, path, monkeypatch)
    assert (out[NEAREST][1]["prim"] == 0).all()
    assert np.array_equal(bits(out[LINEAR][0]), bits(out[NEAREST][0]))
    texels = np.array([tex.rgb[j, i] for j in range(1, 5) for i in range(8)])
    assert np.array_equal(bits(out[LINEAR][0]), bits(texels))


# ---- 4. the linear showcase through every entry point --------------------------------------------------------------------------------
class LinearFlat(UvFlat):
    """test_texture_map_gpu's flattener taught the record kinds 3..5."""

    def pattern(self, p):
        new = p.tag == "uv" and id(p) not in self._pat_ids
        k = super().pattern(p)
        if new:
            for r, f in zip(self.uv[len(self.uv) - len(p.faces):], p.faces):
                r.kind = f.kind_code(p.kind)
        return k


def linear_flatten(world):
    f = LinearFlat()
    for l in world.lights:
        r = ff.RtcLight()
        r.intensity = (C.c_double * 3)(l.intensity.r, l.intensity.g, l.intensity.b)
        r.origin = (C.c_double * 3)(*l.origin[:3])
        f.lights.append(r)
    for e in world.elements:
        f.walk(ff.build(e))
    return f


def test_linear_showcase_identical_everywhere(hip, monkeypatch):
    lib = hip.lib
    c, world = scenes.texture_showcase_linear(64, 48)
    near = scenes.texture_showcase(64, 48)[1]
    sp = Sampling(side=2, jitter=True, seed=9)
    frames, sampled_frames = [], []
    for path in PATHS:
        monkeypatch.setenv("RTC_KERNEL", path)
        a, b = render_world(hip, world, c), render_world(hip, near, c)
        frames.append(a[0])
        for k in ("rays_primary", "rays_shadow", "rays_reflect", "rays_refract", "rays_container"):   # a filter traces no ray
            assert getattr(a[3], k) == getattr(b[3], k), (path, k)
        assert np.array_equal(a[2], b[2]) and a[1].tobytes() == b[1].tobytes()
        assert (bits(a[0]) != bits(b[0])).any(), "the linear showcase is the nearest one"
        nw = hip.build_world(world)
        sampled_frames.append(sampled(lib, bm.scene_of(hip, nw), c, sp, 5))
        nw.close()
    assert np.array_equal(bits(frames[0]), bits(frames[1]))
    assert np.array_equal(bits(sampled_frames[0]), bits(sampled_frames[1])) and np.isfinite(sampled_frames[0]).all()
    monkeypatch.delenv("RTC_KERNEL")
    rgb = frames[0]
    img = Image.par_render(c, world)
    assert np.array_equal(bits(np.asarray(img.pixels).reshape(-1, 3)), bits(rgb))
    flat = linear_flatten(world)
    assert sorted(r.kind for r in flat.uv if r.kind >= 2) == [LINEAR_WRAP_U]
    desc, ext = flat.desc(), flat.ext()
    n = c.hsize * c.vsize
    rc = ff.make_camera(c)
    for path in PATHS:
        monkeypatch.setenv("RTC_KERNEL", path)
        scene = vp()
        assert lib.rtc_scene_create_ext(C.byref(desc), C.byref(ext), 0, C.byref(scene)) == 0, lib.rtc_last_error()
        own = np.empty((n, 3))
        assert lib.rtc_render(scene, C.byref(rc), 5, None, 0, n, own.ctypes.data, None, None) == 0, lib.rtc_last_error()
        assert np.array_equal(bits(own), bits(rgb)), path
        rgb8, q = np.zeros(rgb.size, dtype=np.uint8), np.zeros(rgb.size, dtype=np.uint8)
        assert lib.rtc_render_rgb8(scene, C.byref(rc), 5, rgb8.ctypes.data, None) == 0, lib.rtc_last_error()
        assert lib.rtc_quantize(scene, np.ascontiguousarray(rgb).ctypes.data, rgb.size, q.ctypes.data) == 0, lib.rtc_last_error()
        assert np.array_equal(rgb8, q), path
        own = sampled(lib, scene, c, sp, 5)
        assert np.array_equal(bits(own), bits(sampled_frames[0])), path
        lib.rtc_scene_destroy(scene)
        m = vp()
        devs = (C.c_int * 2)(0, 0)
        assert lib.rtc_multi_create_ext(C.byref(desc), C.byref(ext), devs, 2, C.byref(m)) == 0, lib.rtc_last_error()
        mrgb = np.full((n, 3), np.nan)
        assert lib.rtc_render_multi(m, C.byref(rc), 5, mrgb.ctypes.data, None) == 0, lib.rtc_last_error()
        lib.rtc_multi_destroy(m)
        assert np.array_equal(bits(mrgb), bits(rgb)), path


# ---- 5. creation on the device path -------------------------------------------------------------------------------------------------
def test_creation_limits_and_device_bytes(hip):
    lib = hip.lib
    tex = seeded_texture(3, 4, 3)
    world = flat_world("plane", Matrix.id(), Pattern.texture_map(Matrix.id(), "planar", UvPattern.image(tex)))

    def create(kind, texture=0):
        flat = linear_flatten(world)
        desc, x = flat.desc(), flat.ext()
        x.uv_patterns[0].kind, x.uv_patterns[0].texture = kind, texture
        s = vp()
        rc = lib.rtc_scene_create_ext(C.byref(desc), C.byref(x), 0, C.byref(s))
        size = None
        if rc == 0:
            size = lib.rtc_scene_device_bytes(s)
            lib.rtc_scene_destroy(s)
        else:
            assert lib.rtc_last_error()
        return rc, size
    assert create(6)[0] == 1 and create(-1)[0] == 1
    rc2, bytes2 = create(NEAREST)
    assert rc2 == 0 and bytes2 > 0
    for kind in LINEAR_KINDS:
        assert create(kind) == (0, bytes2), kind
        assert create(kind, 1)[0] == 1 and create(kind, -1)[0] == 1, kind
