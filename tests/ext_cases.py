"""The scenes of the extended oracle's parity tests (test_oracle_ext_cpu.py, test_oracle_ext_gpu.py): worlds that use area lights,
texture maps, light cones, backgrounds and bump records under full lighting and bounces.  Pure scene descriptions; nothing here needs a library."""
import dataclasses
import math
import os

import numpy as np

import build_matrix as bm
import bump_cases as bc
from raytracer_challenge_amd import scenes
from raytracer_challenge_amd.scene import (AreaLight, Background, Bump, Camera, Color, Cone, Element, GroupKind, Material, Matrix, Noise, Pattern, PointLight, ShapeArgs,
                                           SpotLight, Vector, World)
from raytracer_challenge_amd.texture import Texture, UvPattern

P, V, c = Vector.point, Vector.vector, Color.new
plain = Pattern.plain


def seeded_texture(w, h, seed):
    return Texture(np.random.default_rng(seed).uniform(0.05, 0.95, (h, w, 3)))


# ---- the committed showcases and fixtures ------------------------------------------------------------------------------------------
def mirror_area_world():
    """test_area_lights_gpu.mirror_world() with its light as a jittered 3x3 area light."""
    from test_area_lights_gpu import mirror_world
    w = mirror_world()
    l = w.lights[0]
    return World([AreaLight(l.intensity, P(l.origin[0] - 0.75, l.origin[1], l.origin[2] - 0.75), V(1.5, 0.0, 0.0), 3, V(0.0, 0.0, 1.5), 3, jitter=True)], w.elements)


def uv_matrix_world():
    """The `uv` scene of the build matrix with real two-colour checkers, under a gradient background."""
    cam, w = bm.small_world(uv="real")
    bg = Background(Pattern.gradient(Matrix.translation(0.0, -1.0, 0.0) * Matrix.scaling(2.0, 2.0, 2.0) * Matrix.rotation_z(math.pi / 2.0),
                                     plain(c(0.9, 0.8, 0.7)), plain(c(0.1, 0.3, 0.8))), "direction")
    return cam, World(w.lights, w.elements, bg)


# ---- one scene with everything -------------------------------------------------------------------------------------------------------
def everything_world(skybox=True):
    """Every extension in one world, L = 3: a jittered 4x4 area light with a smooth cone, a point light with a hard-edged cone, a plain
    point light; a reflective floor with a 7x5 image on a planar map; a glass-and-mirror sphere with spherical UV checkers whose children
    are a Mixture and a point jitter; a cylinder with a cylindrical align check; a cube-mapped cube with a 1x1 texture on one face; a CSG
    difference, the low teapot, a primitive that casts no shadow; a skybox of six different faces (one an image) -- or, skybox=False, a
    gradient over the ray's direction."""
    lights = [
        AreaLight(c(0.7, 0.7, 0.6), P(-3.0, 6.0, -4.0), V(1.6, 0.0, 0.0), 4, V(0.0, 0.0, 1.6), 4, jitter=True, cone=Cone(V(2.2, -6.0, 3.2), 0.25, 0.55)),
        SpotLight(c(0.5, 0.45, 0.4), P(4.0, 5.0, -3.0), V(-4.0, -5.0, 3.5), 0.45, 0.45),
        PointLight(c(0.3, 0.3, 0.35), P(-1.0, 7.0, -8.0)),
    ]
    floor = Element.plane(ShapeArgs(material=Material(
        pattern=Pattern.texture_map(Matrix.scaling(3.0, 1.0, 3.0), "planar", UvPattern.image(seeded_texture(7, 5, 41))), specular=0.1, reflective=0.35)))
    mix = Pattern.stripes(Matrix.scaling(0.25, 0.25, 0.25), plain(c(0.9, 0.2, 0.1)), plain(c(0.95, 0.8, 0.2)))
    jit = Pattern.point_jitter(Noise.Simplex(0.3), Pattern.ring(Matrix.scaling(0.2, 0.2, 0.2), plain(c(0.1, 0.3, 0.9)), plain(c(0.1, 0.8, 0.7))))
    ball = Element.sphere(ShapeArgs(transform=Matrix.translation(-0.6, 1.0, 0.2), material=Material(
        pattern=Pattern.texture_map(Matrix.rotation_y(0.37) * Matrix.rotation_x(0.21), "spherical", UvPattern.checkers(10.0, 5.0, mix, jit)),
        diffuse=0.5, specular=0.6, reflective=0.4, transparency=0.5, refractive_index=1.4)))
    cols = [plain(c(*m)) for m in ((0.8, 0.8, 0.8), (1, 0, 0), (1, 1, 0), (0, 1, 0), (0, 1, 1))]
    can = Element.cylinder(ShapeArgs(transform=Matrix.translation(2.0, 0.0, 1.2) * Matrix.scaling(0.7, 1.0, 0.7), material=Material(
        pattern=Pattern.texture_map(Matrix.rotation_y(0.13) * Matrix.scaling(1.0, 0.6, 1.0), "cylindrical", UvPattern.align_check(*cols)), diffuse=0.8)), 0.0, 1.6, True)
    one = Texture(np.array([[(0.15, 0.85, 0.55)]]))
    faces = [UvPattern.checkers(2.0, 2.0, plain(c(0.9, 0.9, 0.9)), plain(c(0.2, 0.2, 0.6))), UvPattern.image(one), UvPattern.align_check(*cols),
             UvPattern.checkers(3.0, 1.0, plain(c(0.7, 0.1, 0.6)), plain(c(0.2, 0.9, 0.3))), UvPattern.image(seeded_texture(3, 4, 43)), UvPattern.align_check(*cols[::-1])]
    box = Element.cube(ShapeArgs(transform=Matrix.translation(-2.6, 0.6, 1.6) * Matrix.rotation_y(0.6) * Matrix.scaling(0.6, 0.6, 0.6), material=Material(
        pattern=Pattern.cube_map(Matrix.id(), *faces), diffuse=0.8, specular=0.2)))
    carved = Element.composite(Matrix.translation(0.9, 0.45, -1.6) * Matrix.rotation_y(0.5) * Matrix.scaling(0.45, 0.45, 0.45), None, GroupKind.Difference, [
        Element.cube(ShapeArgs(material=bm.plain(0.9, 0.7, 0.2))), Element.sphere(ShapeArgs(transform=Matrix.scaling(1.3, 1.3, 1.3), material=bm.plain(0.8, 0.1, 0.1, reflective=0.3)))])
    teapot = bm.teapot(-1.9, 0.0, -1.4, 0.1, 0.8, bm.plain(0.85, 0.6, 0.3, specular=0.4))
    ghost = Element.sphere(ShapeArgs(transform=Matrix.translation(0.4, 2.4, 0.6) * Matrix.scaling(0.4, 0.4, 0.4), material=bm.plain(0.6, 0.2, 0.7), casts_shadow=False))
    if skybox:
        sky = [UvPattern.checkers(4.0, 4.0, plain(c(0.2, 0.3, 0.8)), plain(c(0.6, 0.7, 0.95))), UvPattern.image(seeded_texture(6, 4, 47)),
               UvPattern.align_check(*[plain(c(*m)) for m in ((0.3, 0.5, 0.9), (1, 0, 0), (1, 1, 0), (0, 1, 0), (0, 1, 1))]),
               UvPattern.checkers(2.0, 6.0, plain(c(0.9, 0.6, 0.3)), plain(c(0.3, 0.2, 0.5))), UvPattern.checkers(3.0, 3.0, plain(c(0.5, 0.8, 1.0)), plain(c(0.9, 0.95, 1.0))),
               UvPattern.checkers(5.0, 5.0, plain(c(0.2, 0.4, 0.2)), plain(c(0.4, 0.3, 0.1)))]
        bg = Background(Pattern.cube_map(Matrix.rotation_y(0.2), *sky), "cube")
    else:
        bg = Background(Pattern.gradient(Matrix.translation(0.0, -1.0, 0.0) * Matrix.scaling(2.0, 2.0, 2.0) * Matrix.rotation_z(math.pi / 2.0),
                                         plain(c(0.95, 0.9, 0.8)), plain(c(0.2, 0.45, 0.9))), "direction")
    return World(lights, [floor, ball, can, box, carved, teapot, ghost], bg)


def everything_camera(w, h):
    return Camera.new(w, h, 1.0, Camera.transform(P(0.3, 2.6, -7.0), P(-0.2, 0.8, 0.0), V(0.0, 1.0, 0.0)))


# ---- the seventh fuzz wave -----------------------------------------------------------------------------------------------------------
UV_MAPS = ("planar", "spherical", "cylindrical", "cube")
UV_KINDS = ("checkers", "align_check", "image")


def _leaf(rng):
    p = plain(c(*rng.uniform(0.05, 0.95, 3)))
    r = rng.random()
    if r < 0.2:
        return Pattern.checkers(Matrix.scaling(*rng.uniform(0.2, 1.5, 3)), p, plain(c(*rng.uniform(0.05, 0.95, 3))))
    if r < 0.3:
        return Pattern.point_jitter(Noise.Simplex(float(rng.uniform(0.05, 0.4))), Pattern.stripes(Matrix.scaling(0.3, 0.3, 0.3), p, plain(c(*rng.uniform(0.05, 0.95, 3)))))
    return p


def _record(rng, kind):
    if kind == "checkers":
        return UvPattern.checkers(float(rng.integers(1, 9)), float(rng.integers(1, 7)), _leaf(rng), _leaf(rng))
    if kind == "align_check":
        return UvPattern.align_check(*[_leaf(rng) for _ in range(5)])
    return UvPattern.image(seeded_texture(int(rng.integers(1, 10)), int(rng.integers(1, 8)), int(rng.integers(1, 1 << 30))))


def random_uv_pattern(rng, background=False):
    """A UV node drawn over all maps x record kinds, sometimes under a Mixture or a jitter node."""
    mapping = UV_MAPS[int(rng.integers(0, 4))]
    T = Matrix.rotation_y(float(rng.uniform(-1, 1))) * Matrix.rotation_x(float(rng.uniform(-1, 1))) * Matrix.scaling(*rng.uniform(0.5, 2.0, 3))
    if rng.random() < 0.4:
        T = Matrix.translation(*rng.uniform(-0.3, 0.3, 3)) * T
    if mapping == "cube":
        node = Pattern.cube_map(T, *[_record(rng, UV_KINDS[int(rng.integers(0, 3))]) for _ in range(6)])
    else:
        node = Pattern.texture_map(T, mapping, _record(rng, UV_KINDS[int(rng.integers(0, 3))]))
    r = rng.random()
    if r < 0.15:
        return Pattern.blend(Matrix.id(), node, plain(c(*rng.uniform(0.05, 0.95, 3))))
    if r < 0.3:
        return Pattern.point_jitter(Noise.Simplex(float(rng.uniform(0.02, 0.2))), node)
    if r < 0.4 and not background:
        return Pattern.color_jitter(Noise.Simplex(float(rng.uniform(0.02, 0.1))), node)
    return node


def _decorate_elements(rng, elements, share):
    out = []
    for e in elements:
        if e.tag == "shape" and rng.random() < share:
            out.append(dataclasses.replace(e, args=dataclasses.replace(e.args, material=dataclasses.replace(e.args.material, pattern=random_uv_pattern(rng)))))
        elif e.tag == "composite":
            out.append(dataclasses.replace(e, children=tuple(_decorate_elements(rng, e.children, share))))
        else:
            out.append(e)
    return out


def _random_cone(rng, origin, target):
    kind = int(rng.integers(0, 4))
    aim = np.asarray(target, dtype=float) - np.asarray(origin[:3], dtype=float) + rng.uniform(-2.0, 2.0, 3)
    if kind == 0:
        return Cone(V(*aim), math.pi, math.pi)                              # open
    if kind == 1:
        a = float(rng.uniform(0.3, 1.0))
        return Cone(V(*aim), a, a)                                          # hard edge
    if kind == 2:
        a = float(rng.uniform(0.2, 0.8))
        return Cone(V(*aim), a, a + float(rng.uniform(0.1, 0.6)))           # smooth
    return Cone(V(*(-aim)), 0.3, 0.5)                                       # aimed away from the scene


def seventh_wave(seed):
    """A world of the first or second fuzz generator (test_fuzz_parity.random_case), decorated from the seed with area lights, cones,
    UV patterns and a background."""
    from test_fuzz_parity import random_case
    assert seed >= 80000
    rng = np.random.default_rng(seed)
    base = int(rng.integers(1000, 1400)) if rng.random() < 0.5 else int(rng.integers(3000, 3400))
    cam, world, fuel, label = random_case(base, sizes=((48, 27), (64, 36)), counts=(17, 40, 96))
    inv = np.linalg.inv(np.array(cam.transform_matrix.m, dtype=float))
    target = inv[:3, 3] - inv[:3, 2] * 12.0
    lights = []
    for k, l in enumerate(world.lights):
        cone = _random_cone(rng, l.origin, target) if rng.random() < 0.5 else None
        if rng.random() < 0.5:
            us, vs = (16, 1) if (seed + k) % 5 == 0 else (int(rng.choice([1, 2, 3, 4])), int(rng.choice([1, 2, 4])))
            u, v = rng.uniform(-1.5, 1.5, 3), rng.uniform(-1.5, 1.5, 3)
            lights.append(AreaLight(l.intensity, l.origin, V(*u), us, V(*v), vs, jitter=bool(rng.integers(0, 2)), cone=cone))
        elif cone is not None:
            lights.append(SpotLight(l.intensity, l.origin, cone.direction, cone.inner_angle, cone.outer_angle))
        else:
            lights.append(l)
    elements = _decorate_elements(rng, world.elements, 0.2)
    bg, what = None, "none"
    if rng.random() < 0.6:
        k = int(rng.integers(0, 4))
        what = ("plain", "mixture", "uv-spherical", "skybox")[k]
        if k == 0:
            bg = Background(plain(c(*rng.uniform(0.1, 0.9, 3))))
        elif k == 1:
            bg = Background(Pattern.gradient(Matrix.translation(0.0, -1.0, 0.0) * Matrix.scaling(2.0, 2.0, 2.0) * Matrix.rotation_z(math.pi / 2.0),
                                             plain(c(*rng.uniform(0.1, 0.9, 3))), plain(c(*rng.uniform(0.1, 0.9, 3)))), "direction")
        elif k == 2:
            bg = Background(Pattern.texture_map(Matrix.rotation_y(float(rng.uniform(-1, 1))), "spherical", _record(rng, UV_KINDS[int(rng.integers(0, 3))])), "direction")
        else:
            bg = Background(Pattern.cube_map(Matrix.id(), *[_record(rng, UV_KINDS[int(rng.integers(0, 3))]) for _ in range(6)]), "cube")
    if fuel == 0 and seed % 2:
        fuel = int(rng.integers(1, 4))   # the base generators draw fuel 0 for a fifth of their worlds; half of those get bounces here
    if len(lights) > 2:
        fuel = min(fuel, 3)
    fuel = min(fuel, 5)
    n_area = sum(isinstance(l, AreaLight) for l in lights)
    n_cone = sum(getattr(l, "cone", None) is not None for l in lights)
    label = "ext fuzz seed %d (base %d, lights=%d area=%d cones=%d background=%s fuel=%d %dx%d)" % (seed, base, len(lights), n_area, n_cone, what, fuel, cam.hsize, cam.vsize)
    return cam, World(lights, elements, bg), fuel, label


def fuzz_seeds():
    """12 seeds by default; RTC_EXT_FUZZ_SEEDS=<n> [RTC_EXT_FUZZ_FIRST=<seed>] runs n consecutive seeds instead (hunting runs)."""
    if "RTC_EXT_FUZZ_SEEDS" in os.environ:
        first = int(os.environ.get("RTC_EXT_FUZZ_FIRST", "80000"))
        return list(range(first, first + int(os.environ["RTC_EXT_FUZZ_SEEDS"])))
    return list(range(80000, 80012))


RAY_SEEDS = (80001, 80004, 80009)


# ---- the case list of the GPU file (and of the CPU file's tie-share and sensitivity tests) ------------------------------------------
def _showcase(fn, **kw):
    return lambda: fn(96, 54, **kw) + (5,)


def _fixture(world_fn, w=96, h=64):
    from test_area_lights_gpu import camera
    return lambda: (camera(w, h), world_fn(), 5)


def _penumbra():
    from test_area_lights_gpu import penumbra_world
    return penumbra_world(jit=True)


FRAME_CASES = {
    "texture_showcase": _showcase(scenes.texture_showcase),
    "spot_showcase": _showcase(scenes.spot_showcase),
    "sky_showcase": _showcase(scenes.sky_showcase, skybox=False),
    "sky_showcase_skybox": _showcase(scenes.sky_showcase, skybox=True),
    "penumbra_jittered": _fixture(_penumbra),
    "mirror_area_3x3": _fixture(mirror_area_world),
    "uv_matrix_background": lambda: uv_matrix_world() + (5,),
    "everything_64x36": lambda: (everything_camera(64, 36), everything_world(True), 5),
    "everything_13x7": lambda: (everything_camera(13, 7), everything_world(True), 5),
    "everything_direction_64x36": lambda: (everything_camera(64, 36), everything_world(False), 5),
    "everything_direction_13x7": lambda: (everything_camera(13, 7), everything_world(False), 5),
}


# ---- bumped worlds (include/rtc.h rtc_bump) -------------------------------------------------------------------------------------------
EVERYTHING_BUMPS = (Bump.simplex(0.08, 2.0), Bump.fractal(3, 0.15, 1.5), Bump.ripple(0.0, 1.3), Bump.simplex(0.1, 3.0), Bump.fractal(2, 0.2, 1.0), Bump.ripple(0.1, 1.3),
                    Bump.simplex(0.25, 1.5), Bump.fractal(8, 0.1, 4.0))


def bumped_everything_world(skybox=True):
    """everything_world with a record on every material, kinds cycled, in the order the materials are met: the image-mapped floor
    (simplex), the glass-and-mirror sphere (fractal), the cylinder (a ripple of AMPLITUDE 0: v == n keeps its bits inside a running NP
    build), the cube-mapped cube (simplex), the CSG difference's cube (fractal) and sphere (ripple), the teapot's smooth triangles
    (simplex), the primitive that casts no shadow (fractal, 8 octaves)."""
    w = bc.bumped(everything_world(skybox), lambda k: EVERYTHING_BUMPS[k])
    assert [e.args.material.bump.amplitude for e in w.elements[:3]] == [0.08, 0.15, 0.0] and w.elements[5].material.bump.kind == "simplex"
    return w


def np_row_case(row):
    """(camera, world, fuel) of the bumped scene of NP build `row` (rtc_bump_info.trace_build; bump_cases.ROWS; test_bump_gpu.py compares its two paths)."""
    cam, twin = bc.row_world(row)
    world = bc.bumped(twin, bc.mixed)
    return cam, world, 5 if len(world.lights) <= 2 else 3


def steep_world():
    """Amplitude 2.0: one glass-and-mirror sphere (fractal) above one mirror plane (ripple), a jittered 3x3 area light with a smooth cone,
    a Plain background that is not black.  The shading normal faces away from the eye on many pixels (ns . eye < 0): schlick with a
    negative cosine, total internal reflection decided on ns, reflected rays that re-enter their own surface, a light-behind test that
    disagrees with the geometry."""
    light = AreaLight(c(0.9, 0.85, 0.8), P(-3.0, 6.0, -4.0), V(1.5, 0.0, 0.0), 3, V(0.0, 0.0, 1.5), 3, jitter=True, cone=Cone(V(3.0, -5.5, 4.0), 0.3, 0.6))
    ball = Element.sphere(ShapeArgs(transform=Matrix.translation(0.0, 1.1, 0.0) * Matrix.scaling(1.1, 1.1, 1.1), material=Material(
        pattern=plain(c(0.2, 0.25, 0.3)), diffuse=0.3, specular=0.7, shininess=60.0, reflective=0.5, transparency=0.7, refractive_index=1.5, bump=Bump.fractal(2, 2.0, 1.5))))
    floor = Element.plane(ShapeArgs(material=Material(pattern=plain(c(0.35, 0.3, 0.25)), diffuse=0.5, specular=0.4, reflective=0.6, bump=Bump.ripple(2.0, 0.9))))
    return World([light], [floor, ball], Background(plain(c(0.3, 0.45, 0.7))))


def steep_camera():
    return Camera.new(37, 19, 1.0, Camera.transform(P(0.4, 2.2, -5.0), P(0.0, 0.9, 0.0), V(0.0, 1.0, 0.0)))


def eighth_wave(seed):
    """The seventh wave's world of the seed, decorated further from the seed: a record on about a third of the materials (group and OBJ
    materials included), kinds uniform, amplitude from {0, 1e-300, 0.05, 0.3, 2.0}, frequency 10^U(-1, 1.5), octaves from {1, 3, 8}."""
    cam, world, fuel, label = seventh_wave(seed)
    rng = np.random.default_rng([seed, 8])
    n = [0, 0]

    def pick(k):
        n[0] += 1
        if rng.random() >= 1.0 / 3.0:
            return None
        n[1] += 1
        kind = int(rng.integers(0, 3))
        a = float(rng.choice([0.0, 1e-300, 0.05, 0.3, 2.0]))
        f = float(10.0 ** rng.uniform(-1.0, 1.5))
        octaves = int(rng.choice([1, 3, 8]))
        return (Bump.simplex(a, f), Bump.fractal(octaves, a, f), Bump.ripple(a, f))[kind]
    world = bc.bumped(world, pick)
    return cam, world, fuel, label.replace("ext fuzz", "bumped ext fuzz") + " records=%d/%d" % (n[1], n[0])


def bump_fuzz_seeds():
    """The seventh wave's 12 seeds by default; RTC_EXT_BUMP_FUZZ_SEEDS=<n> [RTC_EXT_BUMP_FUZZ_FIRST=<seed>] runs n consecutive seeds instead."""
    if "RTC_EXT_BUMP_FUZZ_SEEDS" in os.environ:
        first = int(os.environ.get("RTC_EXT_BUMP_FUZZ_FIRST", "80000"))
        return list(range(first, first + int(os.environ["RTC_EXT_BUMP_FUZZ_SEEDS"])))
    return list(range(80000, 80012))


# The ripple plane of the hand-made rays: frequency 1 under a transform of powers of two, so that material-space radii 0, 0.5 and 1.0
# (r == 0, g == 1, g == 0) are met exactly: material point p -> world point (2 + 2 px, 0, -1 + 2 pz).
RIPPLE_T = Matrix.translation(2.0, 0.0, -1.0) * Matrix.scaling(2.0, 1.0, 2.0)
RIPPLE_GROUP_T = Matrix.translation(1.0, 0.0, 2.0) * Matrix.scaling(2.0, 2.0, 2.0)
GLASS_AT = (2.0, 1.5, 3.0)


def ripple_plane_world(grouped):
    """A mirror plane with a ripple record (bare: the kplanes shortcut of prepare_state; grouped: under a transformed aggregation group,
    which keeps its children's materials) and a bumped glass sphere, two point lights, a gradient background."""
    mirror = Material(pattern=plain(c(0.3, 0.5, 0.4)), diffuse=0.6, specular=0.3, reflective=0.5, bump=Bump.ripple(0.5, 1.0))
    glass = Material(pattern=plain(c(0.1, 0.1, 0.2)), diffuse=0.2, reflective=0.4, transparency=0.8, refractive_index=1.5, bump=Bump.simplex(0.3, 2.0))
    els = [Element.plane(ShapeArgs(transform=RIPPLE_T, material=mirror)), Element.sphere(ShapeArgs(transform=Matrix.translation(*GLASS_AT), material=glass))]
    if grouped:
        els = [Element.composite(RIPPLE_GROUP_T, None, GroupKind.Aggregation, els)]
    return World(list(bm.LIGHTS), els, uv_matrix_world()[1].background)


def _hand_rays(grouped):
    down = (0.0, -1.0, 0.0)   # (unit directions only: a longer one lifts reflect . eye above 1 and its power out of a colour's range)
    rays = []
    for px, pz in ((0.0, 0.0), (0.5, 0.0), (1.0, 0.0), (0.0, 1.0), (0.0, -0.5), (-1.0, 0.0), (-0.5, 0.0), (1.5, 0.0), (0.25, 0.0), (0.3, 0.4), (0.6, 0.8)):
        X = np.array([2.0 + 2.0 * px, 0.0, -1.0 + 2.0 * pz])
        rays.append(tuple(X + np.array([0.0, 5.0, 0.0])) + down)                     # straight down the material-space y direction
        rays.append(tuple(X - np.array([0.0, 3.0, 0.0])) + (0.0, 1.0, 0.0))          # the same point from below: the plane's inside flip
    rng = np.random.default_rng(5)
    for _ in range(40):                                                             # starting inside the bumped glass sphere
        d = rng.normal(size=3)
        rays.append(tuple(np.array(GLASS_AT) + rng.uniform(-0.5, 0.5, 3)) + tuple(d / np.sqrt((d * d).sum())))
    for d in ((0.0, -1.0, 0.0), (0.0, 1.0, 0.0), (1.0, 0.0, 0.0), (0.0, 0.0, -1.0)):
        rays.append(GLASS_AT + d)                                                   # from its centre
    rays = np.array(rays, dtype=np.float64)
    if grouped:                                                                     # the group's transform on the origins (powers of two: exact)
        rays[:, :3] = rays[:, :3] * 2.0 + np.array([1.0, 0.0, 2.0])
    return rays


BUMP_RAY_WORLDS = ("everything", "open", "ripple_bare", "ripple_grouped")


def bump_ray_sets(name):
    """(world, fuel, {set: rays}) of one bumped world for rtc_trace_rays: cases.edge_rays and cases.special_rays (cone and cylinder
    apexes hand a NaN geometric normal to step 4) and, for the two ripple-plane worlds, the hand-made rays; the open world also takes
    rays that start inside its bumped glass-and-mirror ball."""
    import cases
    seed = 81000 + BUMP_RAY_WORLDS.index(name)
    if name == "everything":
        world = bumped_everything_world(False)
    elif name == "open":
        world = bc.bumped(bc.row_world(6)[1], bc.mixed)
    else:
        world = ripple_plane_world(name == "ripple_grouped")
    points = World([l if isinstance(l, PointLight) else PointLight(l.intensity, getattr(l, "origin", None) or l.corner) for l in world.lights], world.elements)
    edge = cases.edge_rays(768, seed=seed).copy()
    sets = {"edge": edge, "special": cases.special_rays(points, 512, seed=seed)}
    if name == "open":
        rng = np.random.default_rng(seed)
        ball = np.array([1.9 * math.cos(0.3), 0.1, 1.4 * math.sin(0.3)])              # bm.balls: the glass-and-mirror ball, radius 0.55
        d = rng.normal(size=(64, 3))
        sets["inside"] = np.concatenate([ball + rng.uniform(-0.3, 0.3, (64, 3)), d / np.sqrt((d * d).sum(axis=1))[:, None]], axis=1)
    if name.startswith("ripple"):
        sets["hand"] = _hand_rays(name == "ripple_grouped")
    return world, 3, sets


KIND_INDEX = {"simplex": 0, "fractal": 1, "ripple": 2}


def flatten_worlds():
    """{name: (world, [(bump or None, the 16 floats of material_inv) per primitive, depth first])}: what rtw.h says of records and
    materials, on worlds small enough to write the answer down.  Every transform is a translation or a scaling by a power of two, so its
    inverse is exact whichever way a library composes it."""
    import foreign_flattener as ff
    inv = lambda m: ff.inverse(m).flat()  # noqa: E731
    out = {}
    # two shapes that share a material but not the bump (and a third that shares both with the first)
    shared = dict(pattern=plain(c(0.9, 0.2, 0.2)), diffuse=0.7)
    bumps = [Bump.simplex(0.2, 2.0), None, Bump.ripple(0.3, 1.5), Bump.simplex(0.2, 2.0), Bump.simplex(0.2, 4.0)]
    ts = [Matrix.translation(2.0 * k, 0.0, 0.0) for k in range(len(bumps))]
    out["shared_material"] = (World([], [Element.sphere(ShapeArgs(transform=t, material=Material(**shared, bump=b))) for t, b in zip(ts, bumps)]),
                              [(b, inv(t)) for t, b in zip(ts, bumps)])
    # a group's material replaces its children's, records included: with a record of its own, and without one
    kids = lambda: [Element.sphere(ShapeArgs(material=Material(bump=Bump.simplex(0.1, 1.0)))),  # noqa: E731
                    Element.cube(ShapeArgs(transform=Matrix.translation(4.0, 0.0, 0.0), material=Material(bump=Bump.fractal(3, 0.2, 2.0)))), Element.sphere(ShapeArgs(transform=Matrix.scaling(0.5, 0.5, 0.5)))]
    g1, g2, g3 = Matrix.translation(1.0, 2.0, 3.0), Matrix.scaling(2.0, 4.0, 0.5), Matrix.translation(-8.0, 0.0, 0.0)
    whole = Bump.ripple(0.25, 2.0)
    out["group_material"] = (World([], [Element.composite(g1, Material(diffuse=0.5, bump=whole), GroupKind.Aggregation, kids()),
                                        Element.composite(g2, Material(diffuse=0.4), GroupKind.Aggregation, kids()),
                                        Element.composite(g3, None, GroupKind.Aggregation, kids()[:2])]),
                             [(whole, inv(g1))] * 3 + [(None, inv(g2))] * 3 + [(Bump.simplex(0.1, 1.0), inv(g3)), (Bump.fractal(3, 0.2, 2.0), inv(g3 * Matrix.translation(4.0, 0.0, 0.0)))])
    # 300 distinct materials, a record on every odd one: material rows past 255
    els, want = [], []
    for k in range(300):
        t = Matrix.translation(float(k % 20) * 4.0, float(k // 20) * 4.0, 0.0)
        b = (Bump.simplex(0.1 + 0.001 * k, 2.0), Bump.fractal(1 + k % 8, 0.2, 1.0 + 0.01 * k), Bump.ripple(0.05, 0.5 + 0.01 * k))[(k // 2) % 3] if k % 2 else None
        els.append(Element.sphere(ShapeArgs(transform=t, material=Material(pattern=plain(c(k / 300.0, 0.5, 0.25)), diffuse=0.3 + 0.002 * k, bump=b))))
        want.append((b, inv(t)))
    out["many_materials"] = (World([], els), want)
    return out


for _row in sorted(bc.ROWS):
    FRAME_CASES["np_row_%02d" % _row] = (lambda r: lambda: np_row_case(r))(_row)
FRAME_CASES.update({
    "bumped_everything_64x36": lambda: (everything_camera(64, 36), bumped_everything_world(True), 5),
    "bumped_everything_13x7": lambda: (everything_camera(13, 7), bumped_everything_world(True), 5),
    "bumped_everything_direction_64x36": lambda: (everything_camera(64, 36), bumped_everything_world(False), 5),
    "bumped_everything_direction_13x7": lambda: (everything_camera(13, 7), bumped_everything_world(False), 5),
    "bump_showcase": lambda: scenes.bump_showcase(48, 27) + (5,),
    "steep_bumps": lambda: (steep_camera(), steep_world(), 4),
})
BUMPED_CASES = tuple(sorted(n for n in FRAME_CASES if "bump" in n or n.startswith("np_row")))

TRIG_FREE = ()   # every committed frame case holds a spherical or cylindrical map except these
for _name in ("spot_showcase", "sky_showcase", "sky_showcase_skybox", "penumbra_jittered", "mirror_area_3x3", "bump_showcase", "steep_bumps",
              "np_row_00", "np_row_01", "np_row_04", "np_row_06", "np_row_07", "np_row_10"):
    TRIG_FREE += (_name,)


def frame_case(name):
    """(camera, world, fuel) of one committed case."""
    return FRAME_CASES[name]()


def ray_sets(seed):
    """(world, fuel, label, {name: rays}) of one RAY_SEEDS world: cases.edge_rays (axis-parallel and non-unit directions, which
    RTC_BG_DIRECTION uses as they are) plus a few rays of its own -- long axis-parallel directions and one direction with a NaN component,
    which takes the cube face "back" --, and cases.special_rays."""
    import cases
    cam, world, fuel, label = seventh_wave(seed)
    edge = cases.edge_rays(2048, seed=seed).copy()
    edge[:, :3] += np.array([0.0, 3.0, 3.0])
    own = np.array([(0.0, 3.0, 3.0, 0.0, 0.0, 5.0), (0.0, 3.0, 3.0, 0.0, 250.0, 0.0), (1.0, 40.0, 2.0, -3.0, 0.0, 0.0), (0.5, 3.0, 1.0, 1e-3, 2e-3, -1e-3),
                    (0.0, 30.0, 3.0, math.nan, 1.0, 0.5), (0.0, 30.0, 3.0, 0.3, 4.0, 0.1),
                    # exactly diagonal directions that leave the scene upwards: two or three components tie for the cube face
                    (0.0, 60.0, 3.0, 1.0, 1.0, 0.5), (0.0, 60.0, 3.0, -2.0, 2.0, 1.0), (0.0, 60.0, 3.0, 0.25, 0.25, 0.25), (0.0, 60.0, 3.0, -3.0, 3.0, -3.0),
                    (0.0, 60.0, 3.0, 0.5, 1.0, 1.0), (0.0, 60.0, 3.0, 0.5, 1.0, -1.0)])
    points = World([l if isinstance(l, PointLight) else PointLight(l.intensity, getattr(l, "origin", None) or l.corner) for l in world.lights], world.elements)
    return world, min(fuel, 3), label, {"edge": np.concatenate([edge, own]), "special": cases.special_rays(points, 1536, seed=seed)}
