"""Bilinear image-texture lookups (include/rtc.h RTC_UV_IMAGE_LINEAR, _LINEAR_WRAP_U, _LINEAR_WRAP), without a GPU: a Python-float
restatement of the header's rule pinned bit for bit to rtc_texture_sample (the host build of csrc/uv_image.h, the function the kernels
compile), the properties the rule promises, the limits through C, rtw and the Python classes, and the shim's mirrors.
test_texture_filter_gpu.py holds the device to rtc_texture_sample."""
import ctypes as C
import math
import os
import re
import struct

import numpy as np
import pytest

from raytracer_challenge_amd.cabi import RtcTexture, load
from raytracer_challenge_amd import Texture, UvPattern, scenes
from raytracer_challenge_amd.backend import _UvFaceC
from raytracer_challenge_amd.scene import Color, Element, Material, Matrix, Pattern, PointLight, ShapeArgs, Vector, World
from test_texture_map_cpu import as_i32, floor, uv_select

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "raytracer_challenge_amd", "csrc", "librtc_amd.so")
vp = C.c_void_p
NEAREST, LINEAR, LINEAR_WRAP_U, LINEAR_WRAP = 2, 3, 4, 5
LINEAR_KINDS = (LINEAR, LINEAR_WRAP_U, LINEAR_WRAP)
SIZES = [(1, 1), (1, 4), (4, 1), (2, 1), (2, 2), (5, 3), (9, 5), (37, 23)]   # (w, h)


@pytest.fixture(scope="module")
def lib():
    return load(LIB)


def seeded(w, h, seed=7):
    """(h, w, 3) f64 texels, row 0 at the top."""
    return np.ascontiguousarray(np.random.RandomState(seed + 100 * w + h).uniform(0.0, 1.0, size=(h, w, 3)))


class HostTexture:
    """An rtc_texture over a numpy array, and rtc_texture_sample on it."""

    def __init__(self, lib, rgb):
        self.lib, self.rgb = lib, np.ascontiguousarray(rgb, dtype=np.float64)
        self.h, self.w = self.rgb.shape[:2]
        self.c = RtcTexture(self.w, self.h, self.rgb.ctypes.data)
        self.out = (C.c_double * 3)()

    def sample(self, kind, u, v):
        assert self.lib.rtc_texture_sample(C.byref(self.c), kind, u, v, self.out) == 0, self.lib.rtc_last_error()
        return (self.out[0], self.out[1], self.out[2])


# ---- the restatement (one Python-float operation per step of the header's rule) ------------------------------------------------------
def c_rem(k, n):  # C's %: the quotient truncates
    return int(math.fmod(k, n))


def axis(a, n, periodic):
    """(i0, i1, t) of one axis at coordinate a over n texels."""
    if not periodic:
        x = a * float(n - 1)
        f = floor(x)
        t = x - f
        i0 = min(max(as_i32(f), 0), n - 1)
        i1 = min(max(as_i32(f + 1.0), 0), n - 1)
    else:
        x = a * float(n) - 0.5
        f = floor(x)
        t = x - f
        i0 = c_rem(c_rem(as_i32(f), n) + n, n)
        i1 = 0 if i0 + 1 == n else i0 + 1
    if t != t:
        t = 0.0
    return i0, i1, t


def corners(kind, w, h, u, v):
    x0, x1, tx = axis(u, w, kind >= LINEAR_WRAP_U)
    y0, y1, ty = axis(1.0 - v, h, kind == LINEAR_WRAP)
    return x0, x1, tx, y0, y1, ty


def restated(rgb, kind, u, v):
    """The rule on an (h, w, 3) array; kind 2 is the nearest texel of test_texture_map_cpu.py."""
    h, w = rgb.shape[:2]
    if kind == NEAREST:
        class _Uv:
            pass
        q = _Uv()
        q.kind, q.texture = "image", _Uv()
        q.texture.width, q.texture.height = w, h
        _, yi, xi = uv_select(q, u, v)
        return tuple(float(c) for c in rgb[yi, xi])
    x0, x1, tx, y0, y1, ty = corners(kind, w, h, u, v)
    out = []
    for ch in range(3):
        c00, c10, c01, c11 = float(rgb[y0, x0, ch]), float(rgb[y0, x1, ch]), float(rgb[y1, x0, ch]), float(rgb[y1, x1, ch])
        top = c00 + (c10 - c00) * tx
        bot = c01 + (c11 - c01) * tx
        out.append(top + (bot - top) * ty)
    return tuple(out)


def bits(rgb):
    return struct.pack("<3d", *rgb)


BELOW_1, ABOVE_0 = math.nextafter(1.0, 0.0), math.nextafter(0.0, 1.0)
NON_FINITE = [1e300, -1e300, math.inf, -math.inf, math.nan]


def special_values(n):
    s = [0.0, 1.0, BELOW_1, ABOVE_0, -0.25, 1.75] + NON_FINITE
    s += [i / (n - 1) for i in range(n)] if n > 1 else []
    s += [(i + 0.5) / n for i in range(n)]
    return s


def uv_set(w, h, n_random=2000, seed=31):
    """The (u, v) every test here and in test_texture_filter_gpu.py looks up: seeded draws in [0, 1), then the special values of each axis
    against a few of the other's (v's are those of a = 1 - v, so the rows' own centres are met exactly where 1 - v is exact)."""
    rng = np.random.default_rng(seed + 1000 * w + h)
    out = [(float(a), float(b)) for a, b in rng.uniform(0.0, 1.0, (n_random, 2))]
    us, vs = special_values(w), special_values(h) + [1.0 - a for a in special_values(h) if math.isfinite(a) and abs(a) < 1e6]
    few_u, few_v = [0.0, 0.37, BELOW_1, math.nan, -0.25], [0.0, 0.61, 1.0, math.inf, 1.75]
    out += [(u, v) for u in us for v in few_v] + [(u, v) for u in few_u for v in vs]
    out += [(u, v) for u in us[:11] for v in vs[:11]]
    return out


# ---- 1. the restatement against the host function ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("size", SIZES, ids=lambda s: "%dx%d" % s)
def test_restatement_is_rtc_texture_sample_bit_for_bit(lib, size):
    w, h = size
    rgb = seeded(w, h)
    tex = HostTexture(lib, rgb)
    pts = uv_set(w, h)
    assert len(pts) > 2000
    for kind in (NEAREST,) + LINEAR_KINDS:
        for u, v in pts:
            got, want = tex.sample(kind, u, v), restated(rgb, kind, u, v)
            assert bits(got) == bits(want), (size, kind, u, v, got, want)


# ---- 2. properties ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size", SIZES, ids=lambda s: "%dx%d" % s)
def test_every_index_is_in_bounds_and_t_in_the_unit_interval(size):
    w, h = size
    for kind in LINEAR_KINDS:
        for u, v in uv_set(w, h, n_random=300):
            x0, x1, tx, y0, y1, ty = corners(kind, w, h, u, v)
            assert 0 <= x0 < w and 0 <= x1 < w and 0 <= y0 < h and 0 <= y1 < h, (size, kind, u, v)
            assert 0.0 <= tx <= 1.0 and 0.0 <= ty <= 1.0, (size, kind, u, v, tx, ty)
    # the saturating conversions: far outside i32 on both sides, on both kinds of axis
    for a in (1e300, -1e300, 3e9, -3e9, math.inf, -math.inf, math.nan):
        for n in (1, 2, 5, 37, 16384):
            for periodic in (False, True):
                i0, i1, t = axis(a, n, periodic)
                assert 0 <= i0 < n and 0 <= i1 < n and 0.0 <= t <= 1.0, (a, n, periodic)


@pytest.mark.parametrize("size", SIZES, ids=lambda s: "%dx%d" % s)
def test_one_colour_texture_returns_its_bits(lib, size):
    w, h = size
    colour = (0.7, 0.45, 0.2)
    tex = HostTexture(lib, np.broadcast_to(np.array(colour), (h, w, 3)))
    for kind in (NEAREST,) + LINEAR_KINDS:
        for u, v in uv_set(w, h, n_random=300):
            assert bits(tex.sample(kind, u, v)) == bits(colour), (size, kind, u, v)


def test_clamped_axis_at_an_integer_is_the_nearest_texel(lib):
    """9x5: u = i/8 and v = 1 - j/4 are exact, x is exactly i and j, t is 0: kind 3 is kind 2's texel, and so is every clamped axis of
    kind 4 (rows); on its own grid, u = (i + 0.5) / n, a periodic axis gives the texel too."""
    rgb = seeded(9, 5)
    tex = HostTexture(lib, rgb)
    for i in range(9):
        for j in range(5):
            u, v = i / 8.0, 1.0 - j / 4.0
            want = tuple(float(c) for c in rgb[j, i])
            assert bits(tex.sample(NEAREST, u, v)) == bits(want)
            assert bits(tex.sample(LINEAR, u, v)) == bits(want), (i, j)
    for i in range(8):   # (i + 0.5) / 8 is exact: an 8-texel period
        rgb8 = seeded(8, 5)
        t8 = HostTexture(lib, rgb8)
        for j in range(5):
            want = tuple(float(c) for c in rgb8[j, i])
            assert bits(t8.sample(LINEAR_WRAP_U, (i + 0.5) / 8.0, 1.0 - j / 4.0)) == bits(want), (i, j)


def test_the_seam_is_continuous_on_a_periodic_axis_only(lib):
    """u = eps and u = 1 - eps are 2 eps apart across the seam: a periodic u moves the colour by at most 2 eps w max|dtexel| (the lerp's
    slope) plus the rounding of the two x: each is a * n with a off by at most 2^-53 and one rounding of at most ulp(37) / 2 = 2^-48, so
    2^-46 for the pair, times a slope of at most 1 per texel, and three roundings of 2^-53 per lerp: 2^-45 covers it.  A clamped u jumps
    from the first column to the last."""
    w, h = 37, 23
    rgb = seeded(w, h)
    tex = HostTexture(lib, rgb)
    span = float(np.abs(rgb[:, 0, :] - rgb[:, -1, :]).max())
    assert span > 0.5                                       # first and last columns differ
    dmax = float(max(np.abs(np.diff(np.concatenate([rgb, rgb[:, :1]], axis=1), axis=1)).max(), 1e-300))
    for eps in (1e-3, 1e-6, 1e-9, 2.0 ** -40):
        bound = 2.0 * eps * w * dmax + 2.0 ** -45
        worst4 = worst3 = 0.0
        for v in (0.0, 0.31, 0.5, 0.77, 1.0):
            a4, b4 = tex.sample(LINEAR_WRAP_U, eps, v), tex.sample(LINEAR_WRAP_U, 1.0 - eps, v)
            a3, b3 = tex.sample(LINEAR, eps, v), tex.sample(LINEAR, 1.0 - eps, v)
            worst4 = max(worst4, max(abs(p - q) for p, q in zip(a4, b4)))
            worst3 = max(worst3, max(abs(p - q) for p, q in zip(a3, b3)))
        assert worst4 <= bound, (eps, worst4, bound)
        assert worst3 > bound and worst3 > 0.25, (eps, worst3, bound)
    # v is periodic for kind 5 alone
    for eps in (1e-6, 1e-9):
        bound = 2.0 * eps * h * float(np.abs(np.diff(np.concatenate([rgb, rgb[:1]], axis=0), axis=0)).max()) + 2.0 ** -45
        for u in (0.1, 0.5, 0.93):
            a5, b5 = tex.sample(LINEAR_WRAP, u, eps), tex.sample(LINEAR_WRAP, u, 1.0 - eps)
            assert max(abs(p - q) for p, q in zip(a5, b5)) <= bound


# ---- 3. validation ----------------------------------------------------------------------------------------------------------------------
def test_rtc_texture_sample_limits(lib):
    rgb = seeded(2, 2)
    good = RtcTexture(2, 2, rgb.ctypes.data)
    out = (C.c_double * 3)()
    for kind in (2, 3, 4, 5):
        assert lib.rtc_texture_sample(C.byref(good), kind, 0.5, 0.5, out) == 0
    for kind in (6, -1, 1, 0):
        assert lib.rtc_texture_sample(C.byref(good), kind, 0.5, 0.5, out) == 1 and lib.rtc_last_error()
    assert lib.rtc_texture_sample(None, 3, 0.5, 0.5, out) == 1
    assert lib.rtc_texture_sample(C.byref(good), 3, 0.5, 0.5, None) == 1
    for bad in (RtcTexture(0, 2, rgb.ctypes.data), RtcTexture(2, 0, rgb.ctypes.data), RtcTexture(2, 2, None), RtcTexture(16385, 1, rgb.ctypes.data)):
        assert lib.rtc_texture_sample(C.byref(bad), 3, 0.5, 0.5, out) == 1 and lib.rtc_last_error()


def image_world(face):
    pat = Pattern.texture_map(Matrix.id(), "planar", face)
    return World([PointLight(Color.white(), Vector.point(-10, 10, -10))], [Element.plane(ShapeArgs(material=Material(pattern=pat)))])


def test_scene_creation_limits_through_c(lib):
    """rtc_scene_create_ext looks for its device before it validates the records, so without one every call here answers RTC_ERR_DEVICE
    (3) and only the absence of a crash is seen; with one the codes are exact (test_texture_filter_gpu.py asserts them on the device
    path as well).  What needs no device is the same rule in rtw_pattern_uv and rtc_texture_sample, above and below."""
    from test_texture_map_gpu import uv_flatten
    world = image_world(UvPattern.image(Texture(seeded(4, 3))))

    def create(kind, texture=0):
        flat = uv_flatten(world)
        desc, x = flat.desc(), flat.ext()
        x.uv_patterns[0].kind, x.uv_patterns[0].texture = kind, texture
        s = vp()
        rc = lib.rtc_scene_create_ext(C.byref(desc), C.byref(x), 0, C.byref(s))
        if rc == 0:
            lib.rtc_scene_destroy(s)
        else:
            assert lib.rtc_last_error()
        return rc
    refused = (1,) if create(NEAREST) == 0 else (3,)
    accepted = (0,) if refused == (1,) else (3,)
    assert create(6) in refused and create(-1) in refused
    for kind in LINEAR_KINDS:
        assert create(kind, 1) in refused and create(kind, -1) in refused, kind      # texture index out of range
        assert create(kind) in accepted, kind
    assert create(NEAREST, 1) in refused


def test_rtw_pattern_uv_takes_the_linear_kinds_with_a_texture():
    import raytracer_challenge_amd as rt
    lib = rt.hip_backend().lib
    tex = lib.rtw_texture_create(1, 1, (C.c_double * 3)())
    eye = (C.c_double * 16)(*Matrix.id().flat())

    def make(map_kind, kind, texture, n=1):
        faces = (_UvFaceC * n)()
        for k in range(n):
            faces[k].kind, faces[k].width, faces[k].height, faces[k].texture = kind, 1.0, 1.0, texture   # no children: none is read
        return lib.rtw_pattern_uv(map_kind, eye, faces, n)
    for kind in LINEAR_KINDS:
        for map_kind, n in ((0, 1), (1, 1), (2, 1), (3, 6)):
            p = make(map_kind, kind, tex, n)
            assert p, (kind, map_kind, lib.rtw_last_error())
            lib.rtw_pattern_release(p)
        assert make(0, kind, None) is None and "texture" in lib.rtw_last_error().decode()
    assert make(0, 6, tex) is None and "face kind" in lib.rtw_last_error().decode()
    assert make(0, -1, tex) is None and "face kind" in lib.rtw_last_error().decode()
    lib.rtw_texture_release(tex)


def test_python_classes():
    tex = Texture(seeded(4, 3))
    plain = UvPattern.image(tex)
    assert plain == UvPattern("image", texture=tex) and plain.filter == "nearest" and plain.kind_code() == 2      # what they were
    assert UvPattern.image(tex, "nearest", "uv").kind_code("spherical") == 2                                       # nearest ignores wrap
    with pytest.raises(TypeError):
        UvPattern.image(np.zeros((1, 1, 3)), filter="linear")
    for kw in ({"filter": "cubic"}, {"filter": None}, {"filter": "linear", "wrap": "mirror"}, {"wrap": "v"}, {"filter": "Linear"}):
        with pytest.raises(ValueError):
            UvPattern.image(tex, **kw)
    assert [UvPattern.image(tex, "linear", w).kind_code() for w in ("clamp", "u", "uv")] == [3, 4, 5]
    auto = UvPattern.image(tex, filter="linear")
    assert auto.wrap == "auto"
    with pytest.raises(ValueError):
        auto.kind_code()                                     # resolved where the map is known
    want = {"planar": ("uv", 5), "cylindrical": ("uv", 5), "spherical": ("u", 4)}
    for mapping, (wrap, code) in want.items():
        f = Pattern.texture_map(Matrix.id(), mapping, auto).faces[0]
        assert (f.wrap, f.kind_code(mapping), f.texture) == (wrap, code, tex), mapping
    cube = Pattern.cube_map(Matrix.id(), *[auto] * 6)
    assert all((f.wrap, f.kind_code("cube")) == ("clamp", 3) for f in cube.faces)
    # an explicit wrap is kept whatever the map; nearest records and the other kinds pass through as they are
    assert Pattern.texture_map(Matrix.id(), "spherical", UvPattern.image(tex, "linear", "clamp")).faces[0].kind_code("spherical") == 3
    assert Pattern.cube_map(Matrix.id(), *[UvPattern.image(tex, "linear", "uv")] * 6).faces[5].kind_code("cube") == 5
    assert Pattern.texture_map(Matrix.id(), "planar", plain).faces[0] is plain
    chk = UvPattern.checkers(2, 2, Pattern.plain(Color.white()), Pattern.plain(Color.black()))
    assert Pattern.texture_map(Matrix.id(), "planar", chk).faces[0] is chk and chk.kind_code("planar") == 0
    # the backend hands rtw the resolved kind (no device: the world is only described)
    import raytracer_challenge_amd as rt
    hip = rt.hip_backend()
    for face in (auto, UvPattern.image(tex, "linear", "clamp"), plain):
        hip.build_world(image_world(face)).close()
    cam, world = scenes.texture_showcase_linear(16, 12)
    near = scenes.texture_showcase(16, 12)[1]
    lin = [f for e in world.elements for f in e.args.material.pattern.faces if f.kind == "image"]
    assert [(f.filter, f.wrap) for f in lin] == [("linear", "u")]
    assert [f.filter for e in near.elements for f in e.args.material.pattern.faces if f.kind == "image"] == ["nearest"]


# ---- the surfaces of test_texture_filter_gpu.py, checked from the oracle's points alone ---------------------------------------------------
SURFACES = [(0, LINEAR_WRAP), (2, LINEAR_WRAP_U), (3, LINEAR_WRAP), (4, LINEAR)]   # test_texture_map_gpu.CASES: planar, spherical, cylindrical, cube
SURFACE_FRAME = (64, 48)
WRAP_OF = {LINEAR: "clamp", LINEAR_WRAP_U: "u", LINEAR_WRAP: "uv"}


def linear(tex, kind):
    return UvPattern.image(tex, filter="linear", wrap=WRAP_OF[kind])


def floor_ties(face, u, v, eps=1e-9):
    """A floor of the rule lies within eps of (u, v): the x of either axis is within eps of an integer."""
    w, h = face.texture.width, face.texture.height
    code = face.kind_code()
    xs = [u * float(w) - 0.5 if code >= LINEAR_WRAP_U else u * float(w - 1), (1.0 - v) * float(h) - 0.5 if code == LINEAR_WRAP else (1.0 - v) * float(h - 1)]
    return any(abs(a - round(a)) < eps for a in xs if math.isfinite(a))


@pytest.mark.parametrize("surface", range(len(SURFACES)))
def test_threshold_ties_stay_under_the_cap_for_the_cameras_chosen(orc, surface):
    """The GPU test may leave out pixels whose x lies within 1e-9 of a floor threshold (or on the atan2 seam), at most 1 % of the hit
    pixels: from the oracle's render of the Debug points, the restatement alone stays under that cap, with enough hit pixels left."""
    from test_texture_map_cpu import uv_map
    from test_texture_map_gpu import CASES, MAPS, T_PATTERN, cam, flat_world
    case, kind = SURFACES[surface]
    shape, transform, mapping = CASES[case]
    world = flat_world(shape, transform, Pattern.checkers(T_PATTERN, Pattern.debug(), Pattern.debug()))
    pts, hits = orc.render(orc.build_world(world), cam(*SURFACE_FRAME), 5)
    hit = hits["prim"] >= 0
    face_of = linear(Texture(seeded(37, 23)), kind)
    ties = 0
    for i in np.flatnonzero(hit):
        _, u, v = uv_map(MAPS[mapping], *pts[i])
        ties += floor_ties(face_of, u, v) or (mapping in ("spherical", "cylindrical") and abs(pts[i][0]) < 1e-9 and pts[i][2] < 0.0)
    assert hit.sum() > 150 and ties <= 0.01 * hit.sum(), (mapping, int(hit.sum()), ties)


# ---- 4. the shim ------------------------------------------------------------------------------------------------------------------------
def test_shim_mirrors_the_kinds_and_the_host_function():
    h = open(os.path.join(ROOT, "include", "rtc.h")).read()
    rs = open(os.path.join(ROOT, "shim", "gpu.rs")).read()
    for name, value in (("RTC_UV_IMAGE", 2), ("RTC_UV_IMAGE_LINEAR", 3), ("RTC_UV_IMAGE_LINEAR_WRAP_U", 4), ("RTC_UV_IMAGE_LINEAR_WRAP", 5)):
        assert re.search(r"\b%s = %d\b" % (name, value), h), name
        assert "pub const %s: i32 = %d;" % (name, value) in rs, name
    assert "fn rtc_texture_sample(tex: *const RtcTexture, kind: i32, u: f64, v: f64, rgb: *mut f64) -> c_int;" in rs
    assert "int rtc_texture_sample(const rtc_texture* tex, int32_t kind, double u, double v, double rgb[3]);" in h
    from test_shim_layout import c_struct, rust_struct
    for c_name, rs_name in (("rtc_uv_pattern", "RtcUvPattern"), ("rtc_texture", "RtcTexture")):   # the layouts did not move
        assert c_struct(h, c_name) == rust_struct(rs, rs_name), c_name
