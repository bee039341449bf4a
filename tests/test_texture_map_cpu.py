"""Texture mapping (include/rtc.h RTC_PAT_UV), without a GPU: a restatement of the maps and UV patterns pinned to the book's tables,
the PPM reader, argument checks of the Python constructors and of rtw_pattern_uv / rtw_texture_create, the libraries that refuse
texture-mapped worlds, and the shim's mirrors.  test_texture_map_gpu.py holds the device to the restatement."""
import ctypes as C
import math
import os

import numpy as np
import pytest

from raytracer_challenge_amd import Texture, UvPattern, read_ppm
from raytracer_challenge_amd.backend import RtwError, _UvFaceC
from raytracer_challenge_amd.cabi import RtcSceneDesc
from raytracer_challenge_amd.image import ppm_text
from raytracer_challenge_amd.scene import Color, Element, Material, Matrix, Pattern, PointLight, ShapeArgs, Vector, World
from test_shim_layout import c_struct, rust_struct

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MAPS = {"planar": 0, "spherical": 1, "cylindrical": 2, "cube": 3}
LEFT, FRONT, RIGHT, BACK, UP, DOWN = range(6)


# ---- the restatement (one f64 operation per step; math.atan2 / math.acos are the C library's) ----------------------------------
def floor(a):
    return float(np.floor(a))


def m1(a):
    return a - floor(a)


def m2(a):
    return a - 2.0 * floor(a * 0.5)


def rmax(a, b):  # Rust's f64::max: a NaN operand is skipped
    return b if a != a else (a if b != b else (a if a > b else b))


def uv_map(kind, x, y, z):
    """(face, u, v): face = the record's offset from the node's first (a cube map's face in cube_map order, else 0)."""
    if kind == 0:
        return 0, m1(x), m1(z)
    if kind in (1, 2):
        theta = math.atan2(x, z)
        u = 1.0 - (theta / (2.0 * math.pi) + 0.5)
        if kind == 2:
            return 0, u, m1(y)
        r = math.sqrt(x * x + y * y + z * z)
        phi = math.acos(y / r) if -1.0 <= y / r <= 1.0 else math.nan
        return 0, u, 1.0 - phi / math.pi
    c = rmax(rmax(abs(x), abs(y)), abs(z))
    if c == x:
        return RIGHT, m2(1.0 - z) / 2.0, m2(y + 1.0) / 2.0
    if c == -x:
        return LEFT, m2(z + 1.0) / 2.0, m2(y + 1.0) / 2.0
    if c == y:
        return UP, m2(x + 1.0) / 2.0, m2(1.0 - z) / 2.0
    if c == -y:
        return DOWN, m2(x + 1.0) / 2.0, m2(z + 1.0) / 2.0
    if c == z:
        return FRONT, m2(x + 1.0) / 2.0, m2(y + 1.0) / 2.0
    return BACK, m2(1.0 - x) / 2.0, m2(y + 1.0) / 2.0


def as_i32(x):
    if x != x:
        return 0
    if x >= 2147483647.0:
        return 2147483647
    if x <= -2147483648.0:
        return -2147483648
    return int(x)


def wadd(a, b):
    return ((a + b + 2 ** 31) % 2 ** 32) - 2 ** 31


def c_round(x):  # C round: half away from zero
    if x != x or math.isinf(x):
        return x
    t = float(math.trunc(x))
    return t + math.copysign(1.0, x) if abs(x - t) >= 0.5 else t


def uv_select(uv, u, v):
    """The child index a UvPattern selects at (u, v), or ("texel", yi, xi) for an image."""
    if uv.kind == "checkers":
        return 0 if wadd(as_i32(floor(u * uv.width)), as_i32(floor(v * uv.height))) % 2 == 0 else 1
    if uv.kind == "align_check":
        if v > 0.8:
            if u < 0.2:
                return 1
            if u > 0.8:
                return 2
        elif v < 0.2:
            if u < 0.2:
                return 3
            if u > 0.8:
                return 4
        return 0
    w, h = uv.texture.width, uv.texture.height
    xi = min(max(as_i32(c_round(u * float(w - 1))), 0), w - 1)
    yi = min(max(as_i32(c_round((1.0 - v) * float(h - 1))), 0), h - 1)
    return ("texel", yi, xi)


def near_threshold(uv, u, v, eps=1e-9):
    """A decision value of this UvPattern lies within eps of a threshold (an ulp of atan2 / acos may tip it)."""
    if uv.kind == "checkers":
        vals = [u * uv.width, v * uv.height]
        return any(abs(a - round(a)) < eps for a in vals if math.isfinite(a))
    if uv.kind == "align_check":
        return any(abs(a - t) < eps for a in (u, v) for t in (0.2, 0.8))
    w, h = uv.texture.width, uv.texture.height
    vals = [u * float(w - 1), (1.0 - v) * float(h - 1)]
    return any(abs(abs(a - math.trunc(a)) - 0.5) < eps for a in vals if math.isfinite(a))


# ---- the book's tables --------------------------------------------------------------------------------------------------------
S2 = math.sqrt(2.0) / 2.0


@pytest.mark.parametrize("p,uv", [((0, 0, -1), (0.0, 0.5)), ((1, 0, 0), (0.25, 0.5)), ((0, 0, 1), (0.5, 0.5)), ((-1, 0, 0), (0.75, 0.5)),
                                  ((0, 1, 0), (0.5, 1.0)), ((0, -1, 0), (0.5, 0.0)), ((S2, S2, 0), (0.25, 0.75))])
def test_spherical_map(p, uv):
    _, u, v = uv_map(1, *map(float, p))
    assert u == pytest.approx(uv[0], abs=1e-12) and v == pytest.approx(uv[1], abs=1e-12)


@pytest.mark.parametrize("p,uv", [((0.25, 0, 0.5), (0.25, 0.5)), ((0.25, 0, -0.25), (0.25, 0.75)), ((0.25, 0.5, -0.25), (0.25, 0.75)),
                                  ((1.25, 0, 0.5), (0.25, 0.5)), ((0.25, 0, -1.75), (0.25, 0.25)), ((1, 0, -1), (0.0, 0.0)), ((0, 0, 0), (0.0, 0.0))])
def test_planar_map(p, uv):
    assert uv_map(0, *map(float, p))[1:] == uv


@pytest.mark.parametrize("p,uv", [((0, 0, -1), (0.0, 0.0)), ((0, 0.5, -1), (0.0, 0.5)), ((0, 1, -1), (0.0, 0.0)), ((0.70711, 0.5, -0.70711), (0.125, 0.5)),
                                  ((1, 0.5, 0), (0.25, 0.5)), ((0.70711, 0.5, 0.70711), (0.375, 0.5)), ((0, -0.25, 1), (0.5, 0.75)),
                                  ((-0.70711, 0.5, 0.70711), (0.625, 0.5)), ((-1, 1.25, 0), (0.75, 0.25)), ((-0.70711, 0.5, -0.70711), (0.875, 0.5))])
def test_cylindrical_map(p, uv):
    _, u, v = uv_map(2, *map(float, p))
    assert u == pytest.approx(uv[0], abs=1e-5) and v == pytest.approx(uv[1], abs=1e-12)


@pytest.mark.parametrize("p,face", [((-1, 0.5, -0.25), LEFT), ((1.1, -0.75, 0.8), RIGHT), ((0.1, 0.6, 0.9), FRONT), ((-0.7, 0, -2), BACK),
                                    ((0.5, 1, 0.9), UP), ((-0.2, -1.3, 1.1), DOWN)])
def test_cube_face(p, face):
    assert uv_map(3, *map(float, p))[0] == face


@pytest.mark.parametrize("face,p,uv", [
    (FRONT, (-0.5, 0.5, 1), (0.25, 0.75)), (FRONT, (0.5, -0.5, 1), (0.75, 0.25)),
    (BACK, (0.5, 0.5, -1), (0.25, 0.75)), (BACK, (-0.5, -0.5, -1), (0.75, 0.25)),
    (LEFT, (-1, 0.5, -0.5), (0.25, 0.75)), (LEFT, (-1, -0.5, 0.5), (0.75, 0.25)),
    (RIGHT, (1, 0.5, 0.5), (0.25, 0.75)), (RIGHT, (1, -0.5, -0.5), (0.75, 0.25)),
    (UP, (-0.5, 1, -0.5), (0.25, 0.75)), (UP, (0.5, 1, 0.5), (0.75, 0.25)),
    (DOWN, (-0.5, -1, 0.5), (0.25, 0.75)), (DOWN, (0.5, -1, -0.5), (0.75, 0.25))])
def test_cube_uv(face, p, uv):
    assert uv_map(3, *map(float, p)) == (face, uv[0], uv[1])


def test_cube_nan_is_back():
    assert uv_map(3, math.nan, math.nan, math.nan)[0] == BACK


WHITE, BLACK = Pattern.plain(Color.white()), Pattern.plain(Color.black())


@pytest.mark.parametrize("u,v,child", [(0.0, 0.0, 0), (0.5, 0.0, 1), (0.0, 0.5, 1), (0.5, 0.5, 0), (1.0, 1.0, 0)])
def test_uv_checkers(u, v, child):
    assert uv_select(UvPattern.checkers(2, 2, BLACK, WHITE), u, v) == child


@pytest.mark.parametrize("u,v,child", [(0.5, 0.5, 0), (0.1, 0.9, 1), (0.9, 0.9, 2), (0.1, 0.1, 3), (0.9, 0.1, 4), (math.nan, 0.9, 0), (0.1, math.nan, 0)])
def test_align_check(u, v, child):
    assert uv_select(UvPattern.align_check(WHITE, WHITE, WHITE, WHITE, WHITE), u, v) == child


def test_image_lookup_stays_in_bounds():
    t = Texture(np.zeros((3, 5, 3)))
    img = UvPattern.image(t)
    assert uv_select(img, 0.0, 1.0) == ("texel", 0, 0) and uv_select(img, 1.0, 0.0) == ("texel", 2, 4)
    assert uv_select(img, 0.5, 0.5) == ("texel", 1, 2) and uv_select(img, 0.375, 0.5) == ("texel", 1, 2)   # 1.5 rounds away from zero
    for u, v in ((math.nan, math.nan), (math.inf, -math.inf), (-math.inf, math.inf), (-3.0, 7.0)):
        _, yi, xi = uv_select(img, u, v)
        assert 0 <= yi < 3 and 0 <= xi < 5


# ---- PPM -----------------------------------------------------------------------------------------------------------------------
def test_ppm_p3_with_comments_and_free_whitespace():
    data = b"P3\n# a comment\n2 2\n# another\n255\n255 0 0   0 255 0\n\n0 0 255 # trailing\n 127 127 127\n"
    a = read_ppm(data)
    assert a.shape == (2, 2, 3)
    assert np.array_equal(a[0, 0], [1.0, 0.0, 0.0]) and np.array_equal(a[1, 0], [0.0, 0.0, 1.0])
    assert a[1, 1, 0] == 127 / 255.0


def test_ppm_book_scaling():  # canvas_from_ppm: values scaled by maxval
    a = read_ppm(b"P3\n1 1\n100\n100 50 25\n")
    assert np.array_equal(a[0, 0], [1.0, 0.5, 0.25])


def test_ppm_p6_8_and_16_bit():
    raw8 = bytes([255, 0, 128, 1, 2, 3])
    a = read_ppm(b"P6\n2 1\n255\n" + raw8)
    assert np.array_equal(a.reshape(-1), np.array(list(raw8), dtype=np.float64) / 255.0)
    vals = np.array([65535, 0, 256, 1, 2, 3], dtype=">u2")
    b = read_ppm(b"P6 1 2 65535\n" + vals.tobytes())
    assert np.array_equal(b.reshape(-1), vals.astype(np.float64) / 65535.0)
    t = Texture.from_ppm(b"P6\n2 1\n255\n" + raw8)
    assert (t.width, t.height) == (2, 1)


@pytest.mark.parametrize("data", [b"P5\n1 1\n255\n\x00", b"", b"P3\n2 2\n255\n1 2 3\n", b"P6\n2 2\n255\n\x00\x01", b"P3\n1 1\n0\n0 0 0\n",
                                  b"P3\n1 1\n65536\n0 0 0\n", b"P3\n1 1\n255\n1 2 x\n"])
def test_ppm_errors(data):
    with pytest.raises(ValueError):
        read_ppm(data)


def test_ppm_round_trip_through_ppm_text(tmp_path):
    rng = np.random.RandomState(7)
    rgb8 = rng.randint(0, 256, size=(5 * 3 * 3,)).astype(np.uint8)
    text = ppm_text(5, 3, rgb8)
    path = tmp_path / "x.ppm"
    path.write_text(text)
    t = Texture.from_ppm(str(path))
    assert (t.width, t.height) == (5, 3)
    assert np.array_equal(np.round(t.rgb.reshape(-1) * 255.0).astype(np.uint8), rgb8)


# ---- Python constructors ----------------------------------------------------------------------------------------------------------
def test_python_constructor_errors():
    with pytest.raises(ValueError):
        Texture(np.zeros((2, 2)))
    with pytest.raises(ValueError):
        Texture(np.zeros((0, 2, 3)))
    for w, h in ((0, 1), (1, -1), (math.inf, 1), (1, math.nan)):
        with pytest.raises(ValueError):
            UvPattern.checkers(w, h, WHITE, BLACK)
    with pytest.raises(TypeError):
        UvPattern.checkers(1, 1, WHITE, "black")
    with pytest.raises(TypeError):
        UvPattern.align_check(WHITE, WHITE, WHITE, WHITE, None)
    with pytest.raises(TypeError):
        UvPattern.image(np.zeros((1, 1, 3)))
    uv = UvPattern.checkers(1, 1, WHITE, BLACK)
    with pytest.raises(ValueError):
        Pattern.texture_map(Matrix.id(), "cube", uv)
    with pytest.raises(TypeError):
        Pattern.texture_map(Matrix.id(), "planar", WHITE)
    with pytest.raises(TypeError):
        Pattern.cube_map(Matrix.id(), uv, uv, uv, uv, uv, WHITE)
    t = Texture(np.zeros((1, 1, 3)))
    assert t == t and t != Texture(np.zeros((1, 1, 3)))   # identity


# ---- the C API's argument checks (no device needed) -------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    from raytracer_challenge_amd import hip_backend
    return hip_backend().lib


def test_rtw_texture_create_errors(lib):
    rgb = (C.c_double * 12)()
    assert lib.rtw_texture_create(0, 1, rgb) is None and "width" in lib.rtw_last_error().decode()
    assert lib.rtw_texture_create(1, 0, rgb) is None
    assert lib.rtw_texture_create(16385, 1, rgb) is None and "16384" in lib.rtw_last_error().decode()
    assert lib.rtw_texture_create(2, 2, None) is None and "NULL" in lib.rtw_last_error().decode()
    t = lib.rtw_texture_create(2, 2, rgb)
    assert t
    lib.rtw_texture_release(t)


def test_rtw_pattern_uv_errors(lib):
    white = lib.rtw_pattern_plain(1.0, 1.0, 1.0)
    tex = lib.rtw_texture_create(1, 1, (C.c_double * 3)())
    eye = (C.c_double * 16)(*Matrix.id().flat())

    def face(kind=0, w=1.0, h=1.0, texture=None, children=2):
        f = _UvFaceC()
        f.kind, f.width, f.height, f.texture = kind, w, h, texture
        for c in range(children):
            f.child[c] = white
        return f

    def make(kind, faces, n=None):
        arr = (_UvFaceC * max(1, len(faces)))(*faces)
        return lib.rtw_pattern_uv(kind, eye, arr, len(faces) if n is None else n)

    ok = make(0, [face()])
    assert ok
    lib.rtw_pattern_release(ok)
    assert make(4, [face()]) is None and "map kind" in lib.rtw_last_error().decode()
    assert make(-1, [face()]) is None
    assert make(3, [face()]) is None and "6 faces" in lib.rtw_last_error().decode()
    assert make(0, [face(), face()]) is None and "1 face" in lib.rtw_last_error().decode()
    assert make(1, [face(kind=3)]) is None and "face kind" in lib.rtw_last_error().decode()
    for w, h in ((0.0, 1.0), (1.0, -2.0), (math.inf, 1.0), (1.0, math.nan)):
        assert make(0, [face(w=w, h=h)]) is None and "finite" in lib.rtw_last_error().decode()
    assert make(0, [face(children=1)]) is None and "NULL" in lib.rtw_last_error().decode()
    assert make(2, [face(kind=1, children=4)]) is None and "NULL" in lib.rtw_last_error().decode()
    assert make(1, [face(kind=2)]) is None and "texture" in lib.rtw_last_error().decode()
    cube = make(3, [face(kind=2, texture=tex, children=0)] * 6)
    assert cube
    lib.rtw_pattern_release(cube)
    singular = (C.c_double * 16)(*([0.0] * 16))
    assert lib.rtw_pattern_uv(0, singular, (_UvFaceC * 1)(face()), 1) is None and "singular" in lib.rtw_last_error().decode()
    lib.rtw_texture_release(tex)
    lib.rtw_pattern_release(white)


def uv_world():
    pat = Pattern.texture_map(Matrix.scaling(0.5, 0.5, 0.5), "spherical", UvPattern.checkers(4, 2, WHITE, BLACK))
    s = Element.sphere(ShapeArgs(material=Material(pattern=pat)))
    return World([PointLight(Color.white(), Vector.point(-10, 10, -10))], [s])


def test_oracle_refuses_uv_patterns():
    from oracle_lib import oracle
    orc = oracle()
    assert not orc.has_texture_map
    with pytest.raises(RtwError, match="texture-mapped patterns need librtc_amd.so"):
        orc.build_world(uv_world())


def test_emulator_loads_and_names_the_missing_entry_point():
    from emu_lib import emu
    from raytracer_challenge_amd.scene import Camera
    e = emu()
    assert e.has_texture_map
    nw = e.build_world(uv_world())
    cam = Camera.new(4, 4, math.pi / 3.0, Camera.transform(Vector.point(0, 0, -5), Vector.point(0, 0, 0), Vector.vector(0, 1, 0)))
    with pytest.raises(RtwError, match="rtc_scene_create_ext"):
        e.render(nw, cam, 5)


def test_flatten_helpers_refuse_uv_worlds(lib):
    from raytracer_challenge_amd import hip_backend
    nw = hip_backend().build_world(uv_world())
    counts = (C.c_uint32 * 8)()
    assert lib.rtw_world_flatten_counts(nw.handle, counts) != 0
    assert "texture-mapped" in lib.rtw_last_error().decode()
    desc = RtcSceneDesc()
    assert lib.rtw_world_flatten_desc(nw.handle, desc) != 0
    assert "texture-mapped" in lib.rtw_last_error().decode()


# ---- the shim --------------------------------------------------------------------------------------------------------------------
def test_shim_mirrors_the_texture_structs():
    with open(os.path.join(ROOT, "include", "rtc.h")) as f:
        h = f.read()
    with open(os.path.join(ROOT, "shim", "gpu.rs")) as f:
        rs = f.read()
    for c_name, rs_name in (("rtc_uv_pattern", "RtcUvPattern"), ("rtc_texture", "RtcTexture"), ("rtc_scene_ext", "RtcSceneExt")):
        assert c_struct(h, c_name) == rust_struct(rs, rs_name), c_name
    assert "fn rtc_scene_create_ext(" in rs and "fn rtc_multi_create_ext(" in rs
