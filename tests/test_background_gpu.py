"""The scene background (include/rtc.h rtc_background) on an MI355X, both device paths: nothing moves without one, the rule ray by ray
against the numpy restatement of test_background_cpu.py, the path weights, the oracle through a dome it can render, path against path
with real backgrounds, the frame shapes that can go wrong, and every render entry point."""
import ctypes as C
import math

import numpy as np
import pytest

import build_matrix as bm
import foreign_flattener as ff
from foreign_flattener import render_scene
import parity
from raytracer_challenge_amd import scenes
from raytracer_challenge_amd.image import Image
from raytracer_challenge_amd.scene import (Adaptive, Background, Camera, Color, Element, Filter, GroupKind, Material, Matrix, Noise, Pattern, PointLight, Sampling,
                                           ShapeArgs, Vector, World)
from raytracer_challenge_amd.texture import Texture, UvPattern
from test_background_cpu import BG_CUBE, BG_DIRECTION, RtcBackground, RtcBackgroundInfo, background_points

pytestmark = pytest.mark.gpu
PATHS = ["1", "4"]
vp = C.c_void_p
FUEL = 5
SKY = Color(0.25, 0.5, 1.0)
SKY_RGB = np.array([0.25, 0.5, 1.0])


def render_world(hip, world, cam, fuel=FUEL):
    """The same through the Python layer: World(background=) -> rtw -> rtc_scene_create_ext3."""
    lib = hip.lib
    nw = hip.build_world(world)
    out = render_scene(lib, bm.scene_of(hip, nw), cam, fuel)
    nw.close()
    return out


def same_frames(a, b, what, counters=True):
    assert np.array_equal(a[0].view(np.uint64), b[0].view(np.uint64)), "%s: %d pixels differ" % (what, int((a[0].view(np.uint64) != b[0].view(np.uint64)).any(axis=1).sum()))
    assert a[1].tobytes() == b[1].tobytes(), "%s: primary hit records differ" % what
    assert np.array_equal(a[2], b[2]), "%s: hit-tree digests differ" % what
    if counters:
        for k in ("rays_primary", "rays_shadow", "rays_reflect", "rays_refract", "rays_container"):
            assert getattr(a[3], k) == getattr(b[3], k), "%s: %s %d != %d" % (what, k, getattr(a[3], k), getattr(b[3], k))


def with_background(world, background):
    return World(world.lights, world.elements, background)


def background_info(hip, nw):
    lib = hip.lib
    info = RtcBackgroundInfo()
    assert lib.rtc_scene_background_info(bm.scene_of(hip, nw), C.byref(info)) == 0, lib.rtc_last_error()
    return info


def background_colors(hip, nw, dirs):
    lib = hip.lib
    dirs = np.ascontiguousarray(dirs, dtype=np.float64).reshape(-1, 3)
    rgb = np.full((len(dirs), 3), np.nan)
    assert lib.rtc_background_colors(bm.scene_of(hip, nw), dirs.ctypes.data, len(dirs), rgb.ctypes.data) == 0, lib.rtc_last_error()
    return rgb


# ---- the open scene of the oracle link and of the path-against-path cases ------------------------------------------------------------
OPEN_LIGHTS = [PointLight(Color(0.5, 0.5, 0.5), Vector.point(-4.0, 6.5, -5.0)), PointLight(Color(0.5, 0.5, 0.5), Vector.point(5.0, 4.0, -3.0))]


def open_world(background=None, lights=None, pot=True):
    """One reflective floor plane, six balls one of which is glass-and-mirror, a carved CSG cube and the low teapot, under two white lights
    of intensity 0.5 each (L = 2); nothing stands behind them: bm.camera() has the horizon in frame."""
    floor = Element.plane(ShapeArgs(material=bm.plain(0.5, 0.7, 0.45, reflective=0.3, specular=0.2)))
    carved = Element.composite(Matrix.translation(0.0, 0.4, -1.0) * Matrix.rotation_y(0.5) * Matrix.scaling(0.5, 0.5, 0.5), None, GroupKind.Difference, [
        Element.cube(ShapeArgs(material=bm.plain(0.9, 0.7, 0.2))), Element.sphere(ShapeArgs(transform=Matrix.scaling(1.3, 1.3, 1.3), material=bm.plain(0.8, 0.1, 0.1, reflective=0.3)))])
    teapot = bm.teapot(0.3, 0.0, 2.4, 0.12, 0.5, bm.plain(0.85, 0.6, 0.3, specular=0.4))
    return World(list(lights or OPEN_LIGHTS), [floor] + bm.balls(6, glass_mirror=True) + [carved] + ([teapot] if pot else []), background)


def domed(world, c):
    """The world the oracle renders instead: the same plus a sphere of radius 1000 around the origin whose surface shows Plain c whatever
    lights it: ambient 1 and nothing else, so its colour is c*0.5 + c*0.5 = c.  It is the world's LAST primitive."""
    dome = Element.sphere(ShapeArgs(transform=Matrix.scaling(1000.0, 1000.0, 1000.0),
                                    material=Material(pattern=Pattern.plain(c), ambient=1.0, diffuse=0.0, specular=0.0, reflective=0.0, transparency=0.0)))
    return World(world.lights, world.elements + [dome])


# ---- 1. nothing moves without one ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["planes6", "ops12_gated", "uv"])
def test_nothing_moves_without_a_background(hip, name, tmp_path, monkeypatch):
    """planes6: a mesh and six kernel-argument planes, no op reads a record (the background build needs the records: the scene's own kernels must
    not see them); ops12_gated: row 5, LDS tables; uv: wf_shade's UV builds and row 8."""
    cam, world = bm.BY_NAME[name].make(tmp_path)
    black = with_background(world, Background(Pattern.plain(Color.black())))
    lib = hip.lib
    for path in PATHS:
        monkeypatch.setenv("RTC_KERNEL", path)
        nw, nb = hip.build_world(world), hip.build_world(black)
        for count in (False, True):
            a, b = bm.kernel_info(hip, nw, 4, count), bm.kernel_info(hip, nb, 4, count)
            assert bytes(a) == bytes(b), "%s: rtc_scene_kernel_info differs on path 4: %s" % (name, [(f, getattr(a, f), getattr(b, f)) for f, _ in a._fields_ if getattr(a, f) != getattr(b, f)])
        assert lib.rtc_scene_wavefront_lds_bytes(bm.scene_of(hip, nw)) == lib.rtc_scene_wavefront_lds_bytes(bm.scene_of(hip, nb))
        ia, ib = background_info(hip, nw), background_info(hip, nb)
        assert ia.has_background == 0 and ia.trace_build == -1 and ia.wf_background_build == -1 and ia.pattern == -1
        assert ib.has_background == 1 and ib.plain_root == 1 and ib.projection == BG_DIRECTION
        assert ib.trace_build == (2 if name == "uv" else 0) and ib.trace_uv == (1 if name == "uv" else 0) and ib.wf_background_build == (1 if name == "uv" else 0)
        fa, fb = render_scene(lib, bm.scene_of(hip, nw), cam, FUEL), render_scene(lib, bm.scene_of(hip, nb), cam, FUEL)
        same_frames(fb, fa, "%s with a black background, path %s" % (name, path))
        assert fa[3].rays_shadow > 0 and fa[0].max() > 0.0


# ---- 2. the rule, ray by ray ------------------------------------------------------------------------------------------------------------
def missing_rays(n=2000, seed=3):
    """Rays that start in front of a unit sphere at the origin and head away from it, with directions of any length."""
    rng = np.random.default_rng(seed)
    o = np.array([0.0, 0.0, -5.0]) + rng.uniform(-1.5, 1.5, (n, 3))
    d = rng.normal(size=(n, 3))
    d[:, 2] = -np.abs(d[:, 2]) - 0.05
    d *= rng.choice([1e-3, 0.25, 1.0, 7.0, 1e4], (n, 1))          # unnormalised
    d[:8] = [(0.0, 0.0, -1.0), (1.0, 0.0, -1.0), (-2.0, 2.0, -2.0), (0.0, 3.0, -3.0), (0.5, -0.0, -0.5), (-0.0, 0.0, -4.0), (1e-8, 1.0, -1e-8), (3.0, 3.0, -3.0)]
    return np.concatenate([o, d], axis=1)


def lone_sphere(background):
    return World([PointLight(Color.white(), Vector.point(-3.0, 4.0, -6.0))], [Element.sphere(ShapeArgs())], background)


@pytest.mark.parametrize("path", PATHS)
def test_the_rule_ray_by_ray(hip, path, monkeypatch):
    monkeypatch.setenv("RTC_KERNEL", path)
    rays = missing_rays()
    dirs = rays[:, 3:]
    for projection, name in ((BG_DIRECTION, "direction"), (BG_CUBE, "cube")):
        nw = hip.build_world(lone_sphere(Background(Pattern.debug(), name)))
        rgb, hits = hip.color_at(nw, rays, FUEL)
        assert (hits["prim"] == -1).all() and (hits["t"] == 0.0).all()
        want = background_points(projection, dirs)
        # (the pixel is 0.0 + 1.0 * B, the contribution ADDED to the ray tree's sum: a -0.0 of B comes out as +0.0; the rule alone keeps it)
        assert np.array_equal(rgb.view(np.uint64), (0.0 + 1.0 * want).view(np.uint64)), "Debug background, %s, path %s" % (name, path)
        assert np.array_equal(background_colors(hip, nw, dirs).view(np.uint64), want.view(np.uint64)), "rtc_background_colors, %s" % name
        assert background_info(hip, nw).plain_root == 0
        # a Stripes node with a translated and scaled transform over two Debug children: the transformed point, the four rows left to right
        t = Matrix.translation(1.5, -2.0, 0.25) * Matrix.scaling(2.0, 0.5, 4.0)       # powers of two: its inverse is exact by any method
        m = np.array(ff.inverse(t).flat()).reshape(4, 4)
        assert list(m[0]) == [0.5, 0.0, 0.0, -0.75] and list(m[1]) == [0.0, 2.0, 0.0, 4.0] and list(m[2]) == [0.0, 0.0, 0.25, -0.0625]
        nw = hip.build_world(lone_sphere(Background(Pattern.stripes(t, Pattern.debug(), Pattern.debug()), name)))
        p = background_points(projection, dirs)
        moved = np.stack([((m[r, 0] * p[:, 0] + m[r, 1] * p[:, 1]) + m[r, 2] * p[:, 2]) + m[r, 3] * 1.0 for r in range(3)], axis=1)
        rgb, hits = hip.color_at(nw, rays, FUEL)
        assert (hits["prim"] == -1).all()
        assert np.array_equal(rgb.view(np.uint64), (0.0 + 1.0 * moved).view(np.uint64)), "Stripes over Debug, %s, path %s" % (name, path)
        assert np.array_equal(background_colors(hip, nw, dirs).view(np.uint64), moved.view(np.uint64))
    # a ray that hits is no ray of the background's: the sphere's pixels do not depend on it
    cam = Camera.new(48, 32, 0.9, Camera.transform(Vector.point(0, 0, -5), Vector.point(0, 0, 0), Vector.vector(0, 1, 0)))
    a, b = render_world(hip, lone_sphere(None), cam), render_world(hip, lone_sphere(Background(Pattern.debug())), cam)
    on = a[1]["prim"] >= 0
    assert on.sum() > 50 and (~on).sum() > 50 and a[1].tobytes() == b[1].tobytes() and np.array_equal(a[2], b[2])
    assert np.array_equal(a[0][on].view(np.uint64), b[0][on].view(np.uint64)) and (a[0][~on] == 0.0).all()
    same_frames((a[0][on], a[1], a[2], a[3]), (b[0][on], b[1], b[2], b[3]), "the sphere under a Debug background")


# ---- 3. weights ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("path", PATHS)
def test_weights_down_the_ray_tree(hip, path, monkeypatch):
    monkeypatch.setenv("RTC_KERNEL", path)
    lights = [PointLight(Color.white(), Vector.point(-4.0, 6.0, -5.0)), PointLight(Color(0.3, 0.2, 0.9), Vector.point(5.0, 3.0, 2.0))]
    cam = Camera.new(48, 32, 1.0, Camera.transform(Vector.point(0.0, 1.0, -4.0), Vector.point(0.0, 1.0, 0.0), Vector.vector(0, 1, 0)))

    def frame(reflective, fuel):
        mirror = Element.plane(ShapeArgs(material=Material(pattern=Pattern.plain(Color(0.9, 0.1, 0.3)), ambient=0.0, diffuse=0.0, specular=0.0, reflective=reflective)))
        return render_world(hip, World(lights, [mirror], Background(Pattern.plain(SKY))), cam, fuel)
    rgb, hits, _, st = frame(0.5, FUEL)
    on, above = hits["prim"] == 0, hits["prim"] == -1
    assert on.sum() >= 48 * 12 and above.sum() >= 48 * 12 and (on | above).all()
    want = (1.0 * 2.0 * 0.5) * SKY_RGB                          # weight 1.0, L = 2 lights, reflective 0.5: one reflected ray, which misses
    assert (rgb[on] == want).all() and (rgb[above] == SKY_RGB).all()
    assert st.rays_reflect == on.sum() and st.rays_refract == 0
    rgb0 = frame(0.5, 0)[0]
    assert (rgb0[on] == 0.0).all() and (rgb0[above] == SKY_RGB).all()      # fuel 0: no child ray, the plane's own colour is black
    rgb4 = frame(0.25, FUEL)[0]
    assert (rgb4[on] == (1.0 * 2.0 * 0.25) * SKY_RGB).all() and (rgb4[above] == SKY_RGB).all()


# ---- 4. oracle link ---------------------------------------------------------------------------------------------------------------------
def dome_comparison(hits, ref_hits, dome, what, rays=None):
    """A ray whose oracle hit is the dome must be a miss on the device; every other record agrees bit for bit.  One kind of ray the dome
    cannot stand in for the void on: the floor is an unbounded plane, the dome cuts it off at radius 1000, and a ray that skims the floor
    meets it beyond that -- in the open world a hit on the floor (primitive 0) outside the dome, under the dome a hit on the dome.  Such
    rays (given `rays`; returned as the second mask) must hit the floor out there and are left out of the colour comparison."""
    sky = ref_hits["prim"] == dome
    beyond = np.zeros(len(sky), dtype=bool)
    if rays is not None:
        point = rays[:, :3] + rays[:, 3:] * hits["t"][:, None]
        beyond = sky & (hits["prim"] == 0) & (np.sqrt((point * point).sum(1)) > 1000.0)
        sky = sky & ~beyond
    assert (hits["prim"][sky] == -1).all() and (hits["t"][sky] == 0.0).all(), "%s: a ray the oracle sends to the dome hits something on the device" % what
    bad = ((hits["prim"] != ref_hits["prim"]) | (hits["push_idx"] != ref_hits["push_idx"]) | (hits["t"].view(np.uint64) != ref_hits["t"].view(np.uint64))) & ~sky
    bad &= ~beyond
    assert not bad.any(), "%s: %d hit records differ, first at %s: got %s want %s" % (what, int(bad.sum()), np.flatnonzero(bad)[:3], hits[bad][:3], ref_hits[bad][:3])
    return (sky, beyond) if rays is not None else sky


ORACLE_PANIC_CAP = 0.10


@pytest.fixture(scope="module")
def dome_reference(orc):
    """The oracle's frame and rays of the domed world, once for both paths."""
    world = open_world()
    ref_world = domed(world, SKY)
    cam = bm.camera()
    rays = bm.rays_for(world, 1024)
    keep = bm.panic_free(orc, ref_world, rays)
    ref = orc.render(orc.build_world(ref_world), cam, FUEL)
    ref_rays = orc.color_at(orc.build_world(ref_world), rays[keep], FUEL)
    return world, cam, rays, keep, ref, ref_rays


@pytest.mark.parametrize("path", PATHS)
def test_oracle_link_through_a_dome(hip, dome_reference, path, monkeypatch):
    """The oracle renders the same world under a sphere of radius 1000 that shows Plain c under any light; the device renders the world
    with Background(Plain c).  Share of bm.rays_for's 2 048 rays the oracle panics on with the dome in every intersection list, measured
    with the oracle alone on the CPU: 0 of 2 048 = 0.00 %, as without the dome (the cap is 10 %); 751 of them end on the dome.  Largest colour difference measured on an MI355X, both paths: 8.9e-16 over the frame, 4.2e-16 over the rays; every ray that sees
    the dome first is c to the bit (DESIGN.md section 15 says which operation separates the rest)."""
    monkeypatch.setenv("RTC_KERNEL", path)
    world, cam, rays, keep, (ref_rgb, ref_hits), (ref_ray_rgb, ref_ray_hits) = dome_reference
    dome = hip.build_world(domed(world, SKY)).primitive_count - 1
    assert len(rays) == 2048
    left_out = 1.0 - keep.mean()
    print("oracle link: %d of %d explicit rays left out (%.2f %%)" % (int((~keep).sum()), len(keep), 100.0 * left_out))
    assert left_out <= ORACLE_PANIC_CAP
    nw = hip.build_world(with_background(world, Background(Pattern.plain(SKY))))
    rgb, hits = hip.render(nw, cam, FUEL)
    sky = dome_comparison(hits, ref_hits, dome, "frame, path %s" % path)
    assert sky.sum() >= 48 * 4 and (~sky).sum() >= 48 * 16, "the horizon is in frame"
    err = parity.rgb_error(rgb, ref_rgb, "frame, path %s" % path)
    print("oracle link: frame max |dRGB| = %.3e (%d of %d pixels see the dome first)" % (err, int(sky.sum()), len(sky)))
    assert err <= parity.RGB_TOL
    assert (rgb[sky] == SKY_RGB).all()
    rrgb, rhits = hip.color_at(nw, rays[keep], FUEL)
    rsky, beyond = dome_comparison(rhits, ref_ray_hits, dome, "rays, path %s" % path, rays[keep])
    assert (ref_ray_hits["prim"] >= 0).all()        # every kept ray starts inside the dome with a direction: the oracle's ray always ends somewhere
    assert beyond.sum() <= 0.02 * len(beyond)       # (28 of 2 048 with the oracle alone on the CPU: the floor at 3 283 units and farther)
    rerr = parity.rgb_error(rrgb[~beyond], ref_ray_rgb[~beyond], "rays, path %s" % path, rel=True)
    print("oracle link: rays max |dRGB| = %.3e (%d of %d rays see the dome first, %d meet the floor beyond it)" % (rerr, int(rsky.sum()), len(rsky), int(beyond.sum())))
    assert rerr <= parity.RGB_TOL
    assert (rrgb[rsky] == SKY_RGB).all()


# ---- 5. path against path, bit for bit, with real backgrounds ------------------------------------------------------------------------------
TEXELS_4X2 = np.array([[(0.1 * (x + 1), 0.2 + 0.05 * x, 0.9 - 0.1 * x) for x in range(4)], [(0.8 - 0.1 * x, 0.15 * (x + 1), 0.05 + 0.2 * x) for x in range(4)]])
FACE_TEXELS = [np.array([[(0.1 + 0.15 * f, 0.2, 0.3), (0.4, 0.1 + 0.15 * f, 0.6)], [(0.7, 0.8, 0.05 + 0.15 * f), (0.02 * (f + 1), 0.5, 0.95)]]) for f in range(6)]


def real_backgrounds():
    P, c = Pattern, Color
    up = Matrix.translation(0.0, -1.0, 0.0) * Matrix.scaling(2.0001, 2.0001, 2.0001) * Matrix.rotation_z(math.pi / 2.0)
    return [
        ("gradient sky with a transform", Background(P.gradient(up, P.plain(c(0.95, 0.9, 0.8)), P.plain(c(0.2, 0.45, 0.9))))),
        ("3D checkers", Background(P.checkers(Matrix.scaling(0.2, 0.2, 0.2), P.plain(c(0.9, 0.9, 0.2)), P.plain(c(0.1, 0.2, 0.7))))),
        ("fractal-jittered gradient", Background(P.point_jitter(Noise.Fractal(0.6, 3), P.gradient(up, P.plain(c(1.0, 0.6, 0.3)), P.plain(c(0.1, 0.1, 0.5)))))),
        ("spherical image map of 4x2 texels", Background(P.texture_map(Matrix.id(), "spherical", UvPattern.image(Texture(TEXELS_4X2))))),
        ("cube map of six 2x2 images", Background(P.cube_map(Matrix.id(), *[UvPattern.image(Texture(t)) for t in FACE_TEXELS]), "cube")),
    ]


def texel_directions_spherical():
    """(direction, texel) for every texel of the 4x2 map: u = 1 - (atan2(x, z) / 2 pi + 0.5) and v = 1 - acos(y / r) / pi at the texel's
    centre column (the two end columns a little inside, away from atan2's cut) and in the middle of its half of the sphere."""
    out = []
    for yi in range(2):
        for xi in range(4):
            u = min(max(xi / 3.0, 0.05), 0.95)
            theta, phi = 2.0 * math.pi * (0.5 - u), math.pi * (0.25 + 0.5 * yi)
            out.append(((2.5 * math.sin(theta) * math.sin(phi), 2.5 * math.cos(phi), 2.5 * math.cos(theta) * math.sin(phi)), TEXELS_4X2[yi, xi]))
    return out


def texel_directions_cube():
    """(direction, texel) for the four texel centres of each face, from the CUBE map's formulas inverted (include/rtc.h): faces in cube_map
    order left, front, right, back, up, down; directions of length 3.7 times the point on the unit cube."""
    point = [lambda u, v: (-1.0, 2 * v - 1, 2 * u - 1), lambda u, v: (2 * u - 1, 2 * v - 1, 1.0), lambda u, v: (1.0, 2 * v - 1, 1 - 2 * u),
             lambda u, v: (1 - 2 * u, 2 * v - 1, -1.0), lambda u, v: (2 * u - 1, 1.0, 1 - 2 * v), lambda u, v: (2 * u - 1, -1.0, 2 * v - 1)]
    out = []
    for f in range(6):
        for yi, v in ((0, 0.75), (1, 0.25)):        # row 0 is the top row: v near 1
            for xi, u in ((0, 0.25), (1, 0.75)):
                out.append((tuple(3.7 * x for x in point[f](u, v)), FACE_TEXELS[f][yi, xi]))
    return out


@pytest.mark.parametrize("which", range(5))
def test_path_against_path_with_real_backgrounds(hip, which, monkeypatch):
    name, background = real_backgrounds()[which]
    cam = bm.camera()
    frames = []
    for path in PATHS:
        monkeypatch.setenv("RTC_KERNEL", path)
        nw = hip.build_world(open_world(background))
        frames.append(render_scene(hip.lib, bm.scene_of(hip, nw), cam, FUEL))
        rays = bm.rays_for(open_world(), 256)
        frames[-1] += (hip.color_at(nw, rays, FUEL),)
        texels = texel_directions_spherical() if which == 3 else texel_directions_cube() if which == 4 else []
        if texels:
            dirs = np.array([d for d, _ in texels])
            want = np.array([t for _, t in texels])
            assert np.array_equal(background_colors(hip, nw, dirs), want), "%s: texel centres, rtc_background_colors" % name
            up = np.concatenate([np.tile([0.0, 50.0, 0.0], (len(dirs), 1)), dirs], axis=1)     # from high above the scene ...
            up = up[dirs[:, 1] > 0.0]                                                          # ... the rays that do not come down
            got, h = hip.color_at(nw, up, FUEL)
            assert (h["prim"] == -1).all() and np.array_equal(got, want[dirs[:, 1] > 0.0]), "%s: texel centres, traced, path %s" % (name, path)
    same_frames(frames[0], frames[1], "%s, both paths" % name)
    assert np.array_equal(frames[0][4][0].view(np.uint64), frames[1][4][0].view(np.uint64)) and frames[0][4][1].tobytes() == frames[1][4][1].tobytes(), "%s: explicit rays" % name
    sky = frames[0][1]["prim"] == -1
    assert sky.sum() >= 48 * 4 and len(np.unique(frames[0][0][sky], axis=0)) > 1, "%s: the sky is not one colour" % name
    plain = render_world(hip, open_world(), cam)                                                # the same hits as without, other pixels
    assert plain[1].tobytes() == frames[1][1].tobytes() and np.array_equal(plain[2], frames[1][2]) and not np.array_equal(plain[0], frames[1][0])


@pytest.mark.parametrize("name", ["area_kops_real", "uv_area_real", "spot_real", "uv_spot_real"])
def test_every_background_build_of_the_one_kernel_path(hip, name, tmp_path, monkeypatch):
    """BG builds 1, 3, 4 and 5 (rtc_background_info.trace_build; 0 and 2: the tests above): area lights, cones and UV patterns under a gradient sky, the
    one-kernel path's BG build against the wavefront path's kernels."""
    cam, world = bm.BY_NAME[name].make(tmp_path)
    world = World(world.lights, world.elements[:1] + world.elements[2:], real_backgrounds()[0][1])        # without the back wall: the sky is in frame
    frames = []
    for path in PATHS:
        monkeypatch.setenv("RTC_KERNEL", path)
        nw = hip.build_world(world)
        info = background_info(hip, nw)
        assert info.trace_build == {"area_kops_real": 1, "uv_area_real": 3, "spot_real": 4, "uv_spot_real": 5}[name]
        frames.append(render_scene(hip.lib, bm.scene_of(hip, nw), cam, FUEL))
    same_frames(frames[0], frames[1], "%s under a sky, both paths" % name)
    assert (frames[0][1]["prim"] == -1).sum() >= 48 * 2


# ---- 6. shapes that can go wrong ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("path", PATHS)
def test_frame_shapes_and_pixel_lists(hip, path, monkeypatch):
    monkeypatch.setenv("RTC_KERNEL", path)
    background = real_backgrounds()[2][1]
    world = open_world(background)
    nw = hip.build_world(world)
    lib = hip.lib
    monkeypatch.setenv("RTC_KERNEL", "1" if path == "4" else "4")
    other = hip.build_world(world)
    for h, v in ((37, 19), (1, 1)):                                   # tile padding on the wavefront path
        cam = bm.camera(h=h, v=v)
        a, b = render_scene(lib, bm.scene_of(hip, nw), cam, FUEL), render_scene(lib, bm.scene_of(hip, other), cam, FUEL)
        same_frames(a, b, "%dx%d, both paths" % (h, v))
        if h > 1:
            assert 0 < (a[1]["prim"] == -1).sum() < h * v
    cam = bm.camera(h=37, v=19)
    full, full_hits = hip.render(nw, cam, FUEL)
    rng = np.random.default_rng(9)
    idx = rng.integers(0, 37 * 19, 300).astype(np.uint64)             # unordered, with repeats
    assert len(np.unique(idx)) < len(idx)
    rgb, hits = hip.render(nw, cam, FUEL, idx)
    assert np.array_equal(rgb.view(np.uint64), full[idx].view(np.uint64)) and hits.tobytes() == full_hits[idx].tobytes()
    # a frame in which every pixel misses: the camera looks up
    up = Camera.new(48, 32, 0.8, Camera.transform(Vector.point(0.0, 3.0, -6.0), Vector.point(0.0, 40.0, -2.0), Vector.vector(0, 0, 1)))
    a, b = render_scene(lib, bm.scene_of(hip, nw), up, FUEL), render_scene(lib, bm.scene_of(hip, other), up, FUEL)
    same_frames(a, b, "every pixel misses, both paths")
    assert (a[1]["prim"] == -1).all() and a[3].rays_shadow == 0 and a[3].rays_reflect == 0
    rays = hip.camera_rays(up, Sampling()).reshape(-1, 6)
    assert np.array_equal(a[0].view(np.uint64), (0.0 + 1.0 * background_colors(hip, nw, rays[:, 3:])).view(np.uint64))
    # ... and one in which none does: straight down at a matte floor, where the background changes nothing
    matte = World(OPEN_LIGHTS, [Element.plane(ShapeArgs(material=bm.plain(0.5, 0.7, 0.45)))] + bm.balls(6)[:3:2], background)
    down = Camera.new(48, 32, 0.8, Camera.transform(Vector.point(0.0, 6.0, 0.0), Vector.point(0.0, 0.0, 0.0), Vector.vector(0, 0, 1)))
    a, b = render_world(hip, matte, down), render_world(hip, World(matte.lights, matte.elements), down)
    assert (a[1]["prim"] >= 0).all() and a[3].rays_reflect == 0 and a[3].rays_refract == 0
    same_frames(a, b, "no pixel misses: with and without the background")


# ---- 7. every entry point carries it ---------------------------------------------------------------------------------------------------------
def quantised(rgb):
    """Color::clamp: round(min(max(c, 0), 1) * 255), half away from zero."""
    y = np.clip(rgb, 0.0, 1.0) * 255.0
    r = np.floor(y)
    return (r + (y - r >= 0.5)).astype(np.uint8)


@pytest.mark.parametrize("path", PATHS)
def test_every_entry_point_carries_the_background(hip, path, monkeypatch):
    monkeypatch.setenv("RTC_KERNEL", path)
    lib = hip.lib
    background = real_backgrounds()[0][1]
    world = open_world(background)
    cam = bm.camera()
    nw = hip.build_world(world)
    frame, _ = hip.render(nw, cam, FUEL)
    sky = render_world(hip, world, cam)[1]["prim"] == -1
    assert sky.sum() >= 48 * 4 and (frame[sky] > 0.0).all()
    assert np.array_equal(hip.render_sampled(nw, cam, Sampling(1), FUEL).view(np.uint64), frame.view(np.uint64))
    sp = Sampling(2)
    sampled = hip.render_sampled(nw, cam, sp, FUEL)
    assert np.array_equal(hip.render_adaptive(nw, cam, Adaptive(sp, Sampling(3), math.inf), FUEL).view(np.uint64), sampled.view(np.uint64))
    assert np.array_equal(hip.render_filtered(nw, cam, sp, Filter.box(0.5), FUEL).view(np.uint64), sampled.view(np.uint64))
    rgb8 = np.zeros((48 * 32, 3), dtype=np.uint8)
    rc = ff.make_camera(cam)
    assert lib.rtc_render_rgb8(bm.scene_of(hip, nw), C.byref(rc), FUEL, rgb8.ctypes.data, None) == 0, lib.rtc_last_error()
    assert np.array_equal(rgb8, quantised(frame))
    # rtc_scene_create_ext3 / rtc_multi_create_ext3 on a descriptor: a Gradient sky the foreign flattener can emit; device 0 alone
    gradient = Pattern.gradient(Matrix.scaling(2.0, 1.0, 1.0) * Matrix.rotation_z(math.pi / 2.0), Pattern.plain(Color(0.9, 0.8, 0.7)), Pattern.plain(Color(0.1, 0.3, 0.8)))
    plain_world = open_world(pot=False)                    # (the foreign flattener has no OBJ loader)
    flat = ff.flatten(plain_world)
    bg = RtcBackground(flat.pattern(gradient), BG_DIRECTION)
    desc = flat.desc()
    s = vp()
    assert lib.rtc_scene_create_ext3(C.byref(desc), None, None, 0, C.byref(bg), 0, C.byref(s)) == 0, lib.rtc_last_error()
    single = render_scene(lib, s, cam, FUEL)
    lib.rtc_scene_destroy(s)
    through_python = render_world(hip, with_background(plain_world, Background(gradient)), cam)
    same_frames(single, through_python, "ext3 on a descriptor against the Python layer, path %s" % path)
    m, devs = vp(), (C.c_int * 1)(0)
    assert lib.rtc_multi_create_ext3(C.byref(desc), None, None, 0, C.byref(bg), devs, 1, C.byref(m)) == 0, lib.rtc_last_error()
    mrgb = np.full((48 * 32, 3), np.nan)
    assert lib.rtc_render_multi(m, C.byref(rc), FUEL, mrgb.ctypes.data, None) == 0, lib.rtc_last_error()
    lib.rtc_multi_destroy(m)
    assert np.array_equal(mrgb.view(np.uint64), single[0].view(np.uint64))
    # bg == NULL is rtc_scene_create_ext2: the black void
    assert lib.rtc_scene_create_ext3(C.byref(desc), None, None, 0, None, 0, C.byref(s)) == 0, lib.rtc_last_error()
    void = render_scene(lib, s, cam, FUEL)
    lib.rtc_scene_destroy(s)
    same_frames(void, render_world(hip, plain_world, cam), "bg == NULL, path %s" % path)
    assert (void[0][void[1]["prim"] == -1] == 0.0).all() and (void[1]["prim"] == -1).sum() >= 48 * 4


def test_par_render_of_sky_showcase(hip, monkeypatch):
    for skybox in (False, True):
        cam, world = scenes.sky_showcase(96, 54, skybox=skybox)
        img = Image.par_render(cam, world)
        px = np.asarray(img.pixels).reshape(-1, 3)
        assert px.shape == (96 * 54, 3) and np.isfinite(px).all()
        frames = []
        for path in PATHS:
            monkeypatch.setenv("RTC_KERNEL", path)
            frames.append(render_world(hip, world, cam))
        monkeypatch.delenv("RTC_KERNEL")
        same_frames(frames[0], frames[1], "sky_showcase (skybox %s), both paths" % skybox)
        assert np.array_equal(frames[0][0], px)
        sky = frames[0][1]["prim"] == -1
        assert sky.sum() > 96 * 10 and (px[sky].max(axis=1) > 0.05).all()        # no void above the horizon
