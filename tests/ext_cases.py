"""The scenes of the extended oracle's parity tests (test_oracle_ext_cpu.py, test_oracle_ext_gpu.py): worlds that use area lights,
texture maps, light cones and backgrounds under full lighting and bounces.  Pure scene descriptions; nothing here needs a library."""
import dataclasses
import math
import os

import numpy as np

import build_matrix as bm
from raytracer_challenge_amd import scenes
from raytracer_challenge_amd.scene import (AreaLight, Background, Camera, Color, Cone, Element, GroupKind, Material, Matrix, Noise, Pattern, PointLight, ShapeArgs,
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
TRIG_FREE = ()   # every committed frame case holds a spherical or cylindrical map except these
for _name in ("spot_showcase", "sky_showcase", "sky_showcase_skybox", "penumbra_jittered", "mirror_area_3x3"):
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
