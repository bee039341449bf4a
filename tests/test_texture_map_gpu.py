"""Texture mapping (include/rtc.h RTC_PAT_UV) on an MI355X, both device paths.  The oracle restates the reference, which has no texture
mapping, so the tests anchor to it through patterns it can render: with ambient 1 and nothing else a pixel is its pattern colour, a
Checkers(T, Debug, Debug) root shows the point a UV node with transform T sees, and the restatement of test_texture_map_cpu.py says
what that node must yield there."""
import ctypes as C
import math

import numpy as np
import pytest

import foreign_flattener as ff
from parity import assert_parity, oracle_reference
from raytracer_challenge_amd.cabi import RtcSceneExt, RtcTexture, RtcUvPattern
from raytracer_challenge_amd import Texture, UvPattern, scenes
from raytracer_challenge_amd.image import Image
from raytracer_challenge_amd.scene import (AreaLight, Camera, Color, Element, GroupKind, Material, Matrix, Noise, Pattern, PointLight,
                                           ShapeArgs, Vector, World)
from test_area_lights_gpu import ex_lights, render_scene
from test_texture_map_cpu import near_threshold, uv_map, uv_select

pytestmark = pytest.mark.gpu
PATHS = ["1", "4"]
vp = C.c_void_p
MAPS = {"planar": 0, "spherical": 1, "cylindrical": 2, "cube": 3}
KINDS = {"checkers": 0, "align_check": 1, "image": 2}


class UvFlat(ff.Flat):
    """The foreign flattener taught RTC_PAT_UV: records and textures for rtc_scene_create_ext."""

    def __init__(self):
        super().__init__()
        self.uv, self.textures, self._tex = [], [], {}

    def pattern(self, p):
        if p.tag != "uv" or id(p) in self._pat_ids:
            return super().pattern(p)
        recs = []
        for f in p.faces:
            r = RtcUvPattern()
            r.kind, r.width, r.height, r.texture = KINDS[f.kind], f.width, f.height, -1
            r.child = (C.c_int32 * 5)(*([self.pattern(c) for c in f.children] + [-1] * (5 - len(f.children))))
            if f.texture is not None:
                if id(f.texture) not in self._tex:
                    self._tex[id(f.texture)] = len(self.textures)
                    self.textures.append(f.texture)
                r.texture = self._tex[id(f.texture)]
            recs.append(r)
        n = ff.RtcPatternNode()
        n.tag, n.kind, n.left, n.right, n.scale, n.octaves = 4, MAPS[p.kind], len(self.uv), -1, 1.0, 1
        n.transform_inv = (C.c_double * 16)(*ff.inverse(p.transform).flat())
        self.uv += recs
        self.pats.append(n)
        self._pat_ids[id(p)] = len(self.pats) - 1
        return len(self.pats) - 1

    def ext(self, lights=None):
        self._ext_keep = [(RtcUvPattern * max(1, len(self.uv)))(*self.uv), (RtcTexture * max(1, len(self.textures)))(),
                          [np.ascontiguousarray(t.rgb) for t in self.textures]]
        for k, t in enumerate(self.textures):
            self._ext_keep[1][k].width, self._ext_keep[1][k].height, self._ext_keep[1][k].rgb = t.width, t.height, self._ext_keep[2][k].ctypes.data
        x = RtcSceneExt()
        if lights:
            self._ext_keep.append(ex_lights(lights))
            x.n_lights, x.lights = len(lights), self._ext_keep[-1]
        x.n_uv_patterns, x.uv_patterns = len(self.uv), self._ext_keep[0]
        x.n_textures, x.textures = len(self.textures), self._ext_keep[1]
        return x


def uv_flatten(world, with_lights=True):
    f = UvFlat()
    for l in (world.lights if with_lights else []):
        r = ff.RtcLight()
        r.intensity = (C.c_double * 3)(l.intensity.r, l.intensity.g, l.intensity.b)
        r.origin = (C.c_double * 3)(*l.origin[:3])
        f.lights.append(r)
    for e in world.elements:
        f.walk(ff.build(e))
    return f


def cam(w, h, frm=(0.0, 3.0, -6.0), to=(0.0, 0.5, 0.0)):
    return Camera.new(w, h, math.pi / 3.0, Camera.transform(Vector.point(*frm), Vector.point(*to), Vector.vector(0, 1, 0)))


def flat_world(shape, transform, pattern):
    """ambient 1, nothing else: a pixel is its pattern colour (Phong's ambient term times a white light, plus two zeros)"""
    m = Material(pattern=pattern, ambient=1.0, diffuse=0.0, specular=0.0)
    e = {"plane": lambda a: Element.plane(a), "sphere": lambda a: Element.sphere(a), "cube": lambda a: Element.cube(a),
         "cylinder": lambda a: Element.cylinder(a, -1.0, 1.0, True)}[shape](ShapeArgs(transform=transform, material=m))
    return World([PointLight(Color.white(), Vector.point(-10, 10, -10))], [e])


T_PATTERN = Matrix.rotation_y(0.3) * Matrix.rotation_x(-0.2) * Matrix.scaling(0.9, 1.1, 0.8)
CASES = [("plane", Matrix.id(), "planar"), ("cube", Matrix.translation(0, 0.6, 0) * Matrix.rotation_y(0.5), "planar"),
         ("sphere", Matrix.translation(0, 0.8, 0), "spherical"), ("cylinder", Matrix.translation(0, 0.5, 0) * Matrix.rotation_z(0.2), "cylindrical"),
         ("cube", Matrix.translation(0, 0.6, 0) * Matrix.rotation_y(0.5) * Matrix.rotation_x(0.4), "cube")]
COLORS = [Color(0.9, 0.1, 0.1), Color(0.1, 0.8, 0.2), Color(0.2, 0.3, 0.9), Color(0.95, 0.9, 0.1), Color(0.6, 0.1, 0.7)]
W, H = 96, 64


def seeded_texture(seed, w=37, h=23):
    return Texture(np.random.RandomState(seed).uniform(0.0, 1.0, size=(h, w, 3)))


def uv_patterns(kind, children, n, seed=11):
    if kind == "checkers":
        return [UvPattern.checkers(6.0 + k, 3.0 + k, children[0], children[1]) for k in range(n)]
    if kind == "align_check":
        return [UvPattern.align_check(*children[:5]) for _ in range(n)]
    return [UvPattern.image(seeded_texture(seed + k)) for k in range(n)]


def mapped(mapping, faces, T=T_PATTERN):
    return Pattern.cube_map(T, *faces) if mapping == "cube" else Pattern.texture_map(T, mapping, faces[0])


def points(hip, orc, shape, transform, T, c, path):
    """The point every hit pixel's UV node sees, from a Checkers(T, Debug, Debug) render pinned to the oracle."""
    world = flat_world(shape, transform, Pattern.checkers(T, Pattern.debug(), Pattern.debug()))
    assert_parity(hip, orc, world, c, 5, label="debug points %s (RTC_KERNEL=%s)" % (shape, path))
    rgb, hits = hip.render(hip.build_world(world), c, 5)
    return rgb, hits["prim"] >= 0


def expected(mapping, faces, pts, hit, colors):
    """restatement: per hit pixel the colour (child colour or texel), and whether a decision lies within 1e-9 of a threshold"""
    out = np.zeros_like(pts)
    tie = np.zeros(len(pts), dtype=bool)
    for i in np.flatnonzero(hit):
        face, u, v = uv_map(MAPS[mapping], *pts[i])
        uv = faces[face]
        s = uv_select(uv, u, v)
        tie[i] = mapping in ("spherical", "cylindrical") and (near_threshold(uv, u, v) or (abs(pts[i][0]) < 1e-9 and pts[i][2] < 0.0))
        if isinstance(s, tuple):
            out[i] = uv.texture.rgb[s[1], s[2]]
        else:
            out[i] = colors[s]
    return out, tie


def check(rgb, want, hit, tie, label):
    use = hit & ~tie
    bad = use & np.any(rgb != want, axis=1)
    n_tie = int((hit & tie).sum())
    print("%s: %d hit pixels, %d excluded as threshold ties" % (label, int(hit.sum()), n_tie))
    assert n_tie <= 0.01 * hit.sum(), (label, n_tie)
    assert not bad.any(), "%s: %d pixels differ from the restatement, first %s: got %s want %s" % (
        label, int(bad.sum()), np.flatnonzero(bad)[:3], rgb[bad][:3], want[bad][:3])


# ---- 1 + 3. pattern space: plain children and image textures ------------------------------------------------------------------------
@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("case", range(len(CASES)))
def test_uv_node_sees_the_pattern_space_point(hip, orc, path, case, monkeypatch):
    monkeypatch.setenv("RTC_KERNEL", path)
    shape, transform, mapping = CASES[case]
    c = cam(W, H)
    pts, hit = points(hip, orc, shape, transform, T_PATTERN, c, path)
    plains = [Pattern.plain(k) for k in COLORS]
    for kind in ("checkers", "align_check", "image"):
        faces = uv_patterns(kind, plains, 6 if mapping == "cube" else 1)
        rgb, _ = hip.render(hip.build_world(flat_world(shape, transform, mapped(mapping, faces))), c, 5)
        want, tie = expected(mapping, faces, pts, hit, [np.array([k.r, k.g, k.b]) for k in COLORS])
        if mapping in ("planar", "cube"):
            assert not tie.any()
        check(rgb, want, hit, tie, "%s %s on a %s (RTC_KERNEL=%s)" % (kind, mapping, shape, path))


# ---- 2. children are evaluated at the UV node's transformed point -------------------------------------------------------------------
@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("case", [0, 2, 4])
def test_children_see_the_transformed_point(hip, orc, path, case, monkeypatch):
    monkeypatch.setenv("RTC_KERNEL", path)
    shape, transform, mapping = CASES[case]
    c = cam(W, H)
    pts, hit = points(hip, orc, shape, transform, T_PATTERN, c, path)
    P = Pattern.plain
    kids = [Pattern.checkers(Matrix.scaling(0.3, 0.3, 0.3), P(Color(1, 0, 0)), P(Color(0, 0, 1))),
            Pattern.point_jitter(Noise.Simplex(0.2), Pattern.stripes(Matrix.scaling(0.25, 0.25, 0.25), P(Color(0, 1, 0)), P(Color(1, 1, 1)))),
            Pattern.blend(Matrix.id(), Pattern.ring(Matrix.scaling(0.2, 0.2, 0.2), P(Color(1, 0.5, 0)), P(Color(0, 0.5, 1))),
                          Pattern.gradient(Matrix.id(), P(Color(0, 0, 0)), P(Color(1, 1, 1)))),
            P(Color(0.3, 0.3, 0.3)), Pattern.debug()]
    # the oracle-pinned renders of Checkers(T, X, X) for every child X
    refs = []
    for X in kids:
        w = flat_world(shape, transform, Pattern.checkers(T_PATTERN, X, X))
        assert_parity(hip, orc, w, c, 5, label="child reference (RTC_KERNEL=%s)" % path)
        refs.append(hip.render(hip.build_world(w), c, 5)[0])
    for kind in ("checkers", "align_check"):
        faces = uv_patterns(kind, kids, 6 if mapping == "cube" else 1)
        rgb, _ = hip.render(hip.build_world(flat_world(shape, transform, mapped(mapping, faces))), c, 5)
        want = np.zeros_like(rgb)
        tie = np.zeros(len(rgb), dtype=bool)
        for i in np.flatnonzero(hit):
            face, u, v = uv_map(MAPS[mapping], *pts[i])
            want[i] = refs[uv_select(faces[face], u, v)][i]
            tie[i] = mapping in ("spherical", "cylindrical") and (near_threshold(faces[face], u, v) or (abs(pts[i][0]) < 1e-9 and pts[i][2] < 0.0))
        check(rgb, want, hit, tie, "%s children, %s (RTC_KERNEL=%s)" % (kind, mapping, path))


# ---- 4. full shading: a one-colour texture is Plain(c) ------------------------------------------------------------------------------
C0 = Color(0.7, 0.45, 0.2)


def shading_world(pattern_for):
    """Phong lighting, shadows, reflection, refraction, CSG and a group; every surface of colour C0 given by pattern_for(shape kind)."""
    def mat(kind, **kw):
        return Material(pattern=pattern_for(kind), **kw)
    floor = Element.plane(ShapeArgs(material=mat("plane", reflective=0.3, specular=0.2)))
    glass = Element.sphere(ShapeArgs(transform=Matrix.translation(-1.2, 1.0, -0.5), material=mat("sphere", transparency=0.8, reflective=0.3,
                                                                                                   refractive_index=1.5, diffuse=0.2)))
    csg = Element.composite(Matrix.translation(1.3, 1.0, 0.8), None, GroupKind.Difference, [
        Element.sphere(ShapeArgs(material=mat("sphere"))), Element.cube(ShapeArgs(transform=Matrix.translation(0.5, 0.5, -0.5) * Matrix.scaling(0.6, 0.6, 0.6),
                                                                                   material=mat("cube")))])
    group = Element.composite(Matrix.translation(0.0, 0.5, 2.5), None, GroupKind.Aggregation, [
        Element.cylinder(ShapeArgs(transform=Matrix.translation(-0.8, 0, 0) * Matrix.scaling(0.4, 1, 0.4), material=mat("cylinder")), 0.0, 1.0, True),
        Element.triangle(ShapeArgs(material=mat("triangle")), Vector.point(0, 0, 0), Vector.point(1, 1.5, 0), Vector.point(1.5, 0, 0.3))])
    return [floor, glass, csg, group]


def texture_for(kind):
    tex = Texture(np.broadcast_to(np.array([C0.r, C0.g, C0.b]), (5, 7, 3)))
    plain = Pattern.plain(C0)
    if kind == "cube":
        return Pattern.cube_map(T_PATTERN, *([UvPattern.image(tex)] * 3 + [UvPattern.checkers(2, 2, plain, plain)] * 3))
    if kind == "sphere":
        return Pattern.texture_map(T_PATTERN, "spherical", UvPattern.image(tex))
    if kind == "cylinder":
        return Pattern.texture_map(T_PATTERN, "cylindrical", UvPattern.checkers(8, 2, plain, plain))
    return Pattern.texture_map(T_PATTERN, "planar", UvPattern.image(tex) if kind == "plane" else UvPattern.align_check(plain, plain, plain, plain, plain))


@pytest.mark.parametrize("path", PATHS)
def test_one_colour_textures_shade_like_plain(hip, orc, path, monkeypatch):
    monkeypatch.setenv("RTC_KERNEL", path)
    lights = [PointLight(Color(0.9, 0.9, 0.9), Vector.point(-6, 8, -6)), PointLight(Color(0.3, 0.3, 0.4), Vector.point(5, 6, -3))]
    plain_world = World(lights, shading_world(lambda k: Pattern.plain(C0)))
    uv_world = World(lights, shading_world(texture_for))
    c = cam(120, 80, frm=(0.0, 3.5, -7.0), to=(0.0, 0.8, 0.5))
    ref = oracle_reference(orc, plain_world, c, 5)
    assert_parity(hip, orc, uv_world, c, 5, label="textured (RTC_KERNEL=%s)" % path, ref=ref)
    a = hip.render(hip.build_world(uv_world), c, 5)[0]
    b = hip.render(hip.build_world(plain_world), c, 5)[0]
    assert np.array_equal(a.view(np.uint64), b.view(np.uint64))
    # with an area light (the oracle has none): the product's own Plain(c) render, bit for bit
    area = [AreaLight(Color.white(), Vector.point(-3, 6, -3), Vector.vector(2, 0, 0), 3, Vector.vector(0, 0, 2), 3, True)]
    a = hip.render(hip.build_world(World(area, uv_world.elements)), c, 5)[0]
    b = hip.render(hip.build_world(World(area, plain_world.elements)), c, 5)[0]
    assert np.array_equal(a.view(np.uint64), b.view(np.uint64))


# ---- 5. entry points and paths ------------------------------------------------------------------------------------------------------
def test_showcase_1080p_identical_everywhere(hip, monkeypatch):
    lib = hip.lib
    c, world = scenes.texture_showcase(1920, 1080)
    frames = []
    for path in PATHS:
        monkeypatch.setenv("RTC_KERNEL", path)
        frames.append(hip.render(hip.build_world(world), c, 5, want_hits=False)[0])
    assert np.array_equal(frames[0].view(np.uint64), frames[1].view(np.uint64))
    monkeypatch.delenv("RTC_KERNEL")
    rgb = frames[0]
    img = Image.par_render(c, world)
    assert np.array_equal(np.asarray(img.pixels).reshape(-1, 3).view(np.uint64), rgb.view(np.uint64))
    flat = uv_flatten(world)
    desc, ext = flat.desc(), flat.ext()
    scene = vp()
    assert lib.rtc_scene_create_ext(C.byref(desc), C.byref(ext), 0, C.byref(scene)) == 0, lib.rtc_last_error()
    n = c.hsize * c.vsize
    rc = ff.make_camera(c)
    own = np.empty((n, 3))
    assert lib.rtc_render(scene, C.byref(rc), 5, None, 0, n, own.ctypes.data, None, None) == 0, lib.rtc_last_error()
    assert np.array_equal(own.view(np.uint64), rgb.view(np.uint64))
    rgb8, q = np.zeros(rgb.size, dtype=np.uint8), np.zeros(rgb.size, dtype=np.uint8)
    assert lib.rtc_render_rgb8(scene, C.byref(rc), 5, rgb8.ctypes.data, None) == 0, lib.rtc_last_error()
    assert lib.rtc_quantize(scene, np.ascontiguousarray(rgb).ctypes.data, rgb.size, q.ctypes.data) == 0, lib.rtc_last_error()
    assert np.array_equal(rgb8, q)
    lib.rtc_scene_destroy(scene)
    m = vp()
    devs = (C.c_int * 2)(0, 0)
    assert lib.rtc_multi_create_ext(C.byref(desc), C.byref(ext), devs, 2, C.byref(m)) == 0, lib.rtc_last_error()
    mrgb = np.full((n, 3), np.nan)
    assert lib.rtc_render_multi(m, C.byref(rc), 5, mrgb.ctypes.data, None) == 0, lib.rtc_last_error()
    lib.rtc_multi_destroy(m)
    assert np.array_equal(mrgb.view(np.uint64), rgb.view(np.uint64))


@pytest.mark.parametrize("path", PATHS)
def test_create_ext_without_uv_is_create(hip, path, monkeypatch):
    monkeypatch.setenv("RTC_KERNEL", path)
    lib = hip.lib
    for name in ("chapter11_title", "chapter14_hexagon"):
        c, world = getattr(scenes, name)(160, 90)
        flat = ff.flatten(world)
        desc = flat.desc()
        a, b = vp(), vp()
        assert lib.rtc_scene_create(C.byref(desc), 0, C.byref(a)) == 0, lib.rtc_last_error()
        assert lib.rtc_scene_create_ext(C.byref(desc), None, 0, C.byref(b)) == 0, lib.rtc_last_error()
        ra, rb = render_scene(lib, a, c, 5), render_scene(lib, b, c, 5)
        lib.rtc_scene_destroy(a)
        lib.rtc_scene_destroy(b)
        assert np.array_equal(ra[0].view(np.uint64), rb[0].view(np.uint64)) and np.array_equal(ra[2], rb[2]), name
        # lights only: rtc_scene_create_ex
        gflat = ff.flatten(World([], world.elements))
        gdesc = gflat.desc()
        x = RtcSceneExt()
        lx = ex_lights(world.lights)
        x.n_lights, x.lights = len(world.lights), lx
        e1, e2 = vp(), vp()
        assert lib.rtc_scene_create_ex(C.byref(gdesc), lx, len(world.lights), 0, C.byref(e1)) == 0, lib.rtc_last_error()
        assert lib.rtc_scene_create_ext(C.byref(gdesc), C.byref(x), 0, C.byref(e2)) == 0, lib.rtc_last_error()
        r1, r2 = render_scene(lib, e1, c, 5), render_scene(lib, e2, c, 5)
        lib.rtc_scene_destroy(e1)
        lib.rtc_scene_destroy(e2)
        assert np.array_equal(r1[0].view(np.uint64), r2[0].view(np.uint64)) and np.array_equal(r1[2], r2[2]), name
        assert np.array_equal(r1[0].view(np.uint64), ra[0].view(np.uint64)), name


# ---- 6. validation ------------------------------------------------------------------------------------------------------------------
def test_texture_validation(hip):
    lib = hip.lib
    P = Pattern.plain
    tex = seeded_texture(3, 4, 3)
    faces = [UvPattern.checkers(2, 2, P(Color.white()), P(Color.black()))] * 3 + [UvPattern.image(tex)] * 3
    world = World([PointLight(Color.white(), Vector.point(-10, 10, -10))],
                  [Element.cube(ShapeArgs(material=Material(pattern=Pattern.cube_map(Matrix.id(), *faces))))])

    def create(mutate=None, ext=True):
        flat = uv_flatten(world)
        desc, x = flat.desc(), flat.ext()
        if mutate:
            mutate(flat, desc, x)
        s = vp()
        rc = lib.rtc_scene_create_ext(C.byref(desc), C.byref(x) if ext else None, 0, C.byref(s))
        msg = (lib.rtc_last_error() or b"").decode()
        if rc == 0:
            lib.rtc_scene_destroy(s)
        else:
            assert msg, rc
        return rc

    def uvnode(flat):
        return [k for k, n in enumerate(flat.pats) if n.tag == 4][0]

    def setattr_node(field, value):
        def m(flat, desc, x):
            setattr(desc.pattern_nodes[uvnode(flat)], field, value)
        return m

    def setattr_rec(k, field, value):
        def m(flat, desc, x):
            setattr(x.uv_patterns[k], field, value)
        return m

    assert create() == 0
    assert create(ext=False) == 1                                                # a tag-4 node in a plain descriptor
    assert create(lambda f, d, x: setattr(x, "n_uv_patterns", 0)) == 1           # no records
    assert create(lambda f, d, x: setattr(x, "n_uv_patterns", 5)) == 1           # left + 6 > records
    assert create(setattr_node("left", 1)) == 1
    assert create(setattr_node("left", -1)) == 1
    assert create(setattr_node("kind", 4)) == 1                                  # unknown map
    assert create(setattr_rec(0, "kind", 3)) == 1                                # unknown UV kind
    assert create(setattr_rec(0, "width", 0.0)) == 1 and create(setattr_rec(1, "height", math.inf)) == 1 and create(setattr_rec(2, "width", math.nan)) == 1
    assert create(lambda f, d, x: x.uv_patterns[0].child.__setitem__(1, 99)) == 1   # child out of range
    assert create(setattr_rec(3, "texture", 1)) == 1 and create(setattr_rec(4, "texture", -1)) == 1
    assert create(lambda f, d, x: setattr(x.textures[0], "width", 0)) == 1
    assert create(lambda f, d, x: setattr(x.textures[0], "rgb", None)) == 1

    def cycle(flat, desc, x):   # a UV child naming the UV node itself
        x.uv_patterns[0].child[0] = uvnode(flat)
    assert create(cycle) == 1
    big = np.zeros((1, 16385, 3))
    assert create(lambda f, d, x: (setattr(x.textures[0], "width", 16385), setattr(x.textures[0], "height", 1),
                                   setattr(x.textures[0], "rgb", big.ctypes.data))) == 2
    # more than 2^26 texels: two textures of 8192 x 4097 (their rgb is never read: the limit is checked before the copy)
    t2 = np.zeros(3, dtype=np.float64)

    def too_many(flat, desc, x):
        arr = (RtcTexture * 2)()
        for k in range(2):
            arr[k].width, arr[k].height, arr[k].rgb = 8192, 4097, t2.ctypes.data
        flat._ext_keep.append(arr)
        x.n_textures, x.textures = 2, arr
    assert create(too_many) == 2
