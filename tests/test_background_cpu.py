"""The scene background (include/rtc.h rtc_background), the parts that need no GPU: a numpy restatement of the projection rule against
rtc_background_point bit for bit, the limits (through C where the library checks them before it needs a device, and through the Python
classes), the refusals of the oracle and of the emulator, the exports and the Rust mirror."""
import ctypes as C
import math
import os

import numpy as np
import pytest

import foreign_flattener as ff
from raytracer_challenge_amd.cabi import RtcBackground, RtcBackgroundInfo, load
from raytracer_challenge_amd.backend import RtwError
from raytracer_challenge_amd.scene import (Background, Camera, Color, Element, Matrix, Pattern, PointLight, ShapeArgs, Vector, World)
from test_shim_layout import c_struct, rust_struct

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "raytracer_challenge_amd", "csrc", "librtc_amd.so")
vp = C.c_void_p
BG_DIRECTION, BG_CUBE = 0, 1


# ---- the numpy restatement of the projection rule (shared with test_background_gpu.py) -------------------------------------------------
def background_points(projection, dirs):
    """include/rtc.h rtc_background: DIRECTION is the direction as it is; CUBE divides it by c = max(|dx|, |dy|, |dz|), a max that skips a
    NaN operand (numpy's fmax), one division per component."""
    d = np.ascontiguousarray(dirs, dtype=np.float64).reshape(-1, 3)
    if projection == BG_DIRECTION:
        return d.copy()
    a = np.abs(d)
    c = np.fmax(np.fmax(a[:, 0], a[:, 1]), a[:, 2])
    with np.errstate(all="ignore"):
        return d / c[:, None]


def lib_points(lib, projection, dirs):
    out = np.empty((len(dirs), 3))
    for k, d in enumerate(np.ascontiguousarray(dirs, dtype=np.float64).reshape(-1, 3)):
        p = (C.c_double * 3)()
        assert lib.rtc_background_point(projection, (C.c_double * 3)(*d), p) == 0, lib.rtc_last_error()
        out[k] = list(p)
    return out


def same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.uint64), np.ascontiguousarray(b).view(np.uint64))


def edge_directions():
    nan, inf = math.nan, math.inf
    return np.array([
        (1.0, 1.0, 0.5), (-2.0, 2.0, 1.0), (3.0, -3.0, -3.0), (0.25, 0.25, 0.25),           # ties between components, of either sign
        (0.0, 1.0, 0.0), (-0.0, -1.0, 0.0), (0.0, -0.0, 5.0), (-0.0, 0.0, -1e-300),          # signed zeros beside one component
        (0.0, 0.0, 0.0), (-0.0, -0.0, -0.0),                                                  # the zero vector: 0 / 0
        (nan, 1.0, 2.0), (1.0, nan, -2.0), (nan, nan, 3.0), (nan, nan, nan),                  # NaN components are skipped by the max
        (inf, 1.0, 2.0), (-inf, inf, 0.0), (1.0, 2.0, -inf), (inf, nan, 1.0),                 # inf / inf is NaN, x / inf is 0
        (1e-310, 2e-310, -3e-310), (1e308, -1.7e308, 5e307), (5e-324, 0.0, 0.0),              # denormals and the range's end
    ])


def test_restated_point_is_rtc_background_point_bit_for_bit():
    lib = load(LIB)
    rng = np.random.default_rng(2026)
    unit = rng.normal(size=(300, 3))
    unit /= np.linalg.norm(unit, axis=1, keepdims=True)
    scaled = rng.normal(size=(300, 3)) * rng.choice([1e-6, 0.01, 1.0, 37.5, 1e9], (300, 1))   # unnormalised, of any scale
    for dirs in (unit, scaled, edge_directions()):
        for projection in (BG_DIRECTION, BG_CUBE):
            assert same_bits(lib_points(lib, projection, dirs), background_points(projection, dirs)), projection
    # what the restatement itself says at the edges
    cube = background_points(BG_CUBE, edge_directions())
    assert list(cube[0]) == [1.0, 1.0, 0.5] and list(cube[1]) == [-1.0, 1.0, 0.5] and list(cube[2]) == [1.0, -1.0, -1.0]
    assert np.isnan(cube[8]).all() and np.isnan(cube[9]).all()                                 # the zero vector
    assert np.isnan(cube[10][0]) and list(cube[10][1:]) == [0.5, 1.0]                          # a NaN component stays, the others are scaled
    assert np.isnan(cube[13]).all()
    assert np.isnan(cube[14][0]) and list(cube[14][1:]) == [0.0, 0.0]                          # inf / inf; finite / inf
    assert math.copysign(1.0, cube[5][0]) == -1.0 and cube[5][1] == -1.0                       # -0.0 / 1.0 keeps its sign
    # on the cube's surface: the largest component is exactly +-1 (x / x), every other within [-1, 1]
    on = background_points(BG_CUBE, scaled)
    assert (np.abs(on).max(axis=1) == 1.0).all() and (np.abs(on) <= 1.0).all()
    # the direction projection does not normalise
    assert same_bits(background_points(BG_DIRECTION, scaled), scaled)


def test_point_refuses_null_and_unknown_projections():
    lib = load(LIB)
    d, p = (C.c_double * 3)(1.0, 2.0, 3.0), (C.c_double * 3)()
    assert lib.rtc_background_point(2, d, p) == 1 and b"projection" in lib.rtc_last_error()
    assert lib.rtc_background_point(-1, d, p) == 1
    assert lib.rtc_background_point(BG_CUBE, None, p) == 1 and lib.rtc_background_point(BG_CUBE, d, None) == 1
    assert lib.rtc_background_colors(None, None, 0, None) == 1
    assert lib.rtc_scene_background_info(None, None) == 1


# ---- limits -----------------------------------------------------------------------------------------------------------------------
def floor_world(background=None):
    return World([PointLight(Color.white(), Vector.point(0, 5, 0))], [Element.plane(ShapeArgs())], background)


def test_limits_through_c_need_no_device():
    """The background's own numbers are validated before the device is looked for: every limit answers RTC_ERR_INVALID (1) here, where a
    valid background gets as far as RTC_ERR_DEVICE (3) on a machine without one (or succeeds on one with)."""
    lib = load(LIB)
    flat = ff.flatten(floor_world())
    sky = flat.pattern(Pattern.gradient(Matrix.id(), Pattern.plain(Color(1, 1, 1)), Pattern.plain(Color(0, 0, 1))))
    desc = flat.desc()
    n_nodes = desc.n_pattern_nodes
    assert sky == n_nodes - 1
    devs = (C.c_int * 1)(0)

    def create(bg, multi=False):
        s = vp()
        rc = (lib.rtc_multi_create_ext3(C.byref(desc), None, None, 0, bg, devs, 1, C.byref(s)) if multi else
              lib.rtc_scene_create_ext3(C.byref(desc), None, None, 0, bg, 0, C.byref(s)))
        if rc == 0:
            (lib.rtc_multi_destroy if multi else lib.rtc_scene_destroy)(s)
        return rc
    bad = {
        "pattern index one past the end": RtcBackground(n_nodes, BG_DIRECTION),
        "negative pattern index": RtcBackground(-1, BG_CUBE),
        "a huge pattern index": RtcBackground(2 ** 31 - 1, BG_DIRECTION),
        "unknown projection": RtcBackground(sky, 2),
        "negative projection": RtcBackground(sky, -1),
    }
    for multi in (False, True):
        for why, bg in bad.items():
            assert create(C.byref(bg), multi) == 1, (why, multi)
            assert b"background" in lib.rtc_last_error(), why
        for bg in (RtcBackground(sky, BG_DIRECTION), RtcBackground(0, BG_CUBE), RtcBackground(n_nodes - 1, BG_CUBE)):
            assert create(C.byref(bg), multi) in (0, 3), multi
        assert create(None, multi) in (0, 3)                                       # bg == NULL is rtc_scene_create_ext2
    s = vp()
    assert lib.rtc_scene_create_ext3(None, None, None, 0, C.byref(bad["unknown projection"]), 0, C.byref(s)) == 1   # a NULL descriptor


def test_world_background_type_errors():
    sky = Pattern.plain(Color(0.2, 0.4, 0.9))
    assert World().background is None and floor_world().background is None        # existing constructions are unchanged
    assert World([], []) == World([], [], None)
    b = Background(sky)
    assert b.projection == "direction" and Background(sky, "cube").projection == "cube"
    assert floor_world(b).background is b
    with pytest.raises(Exception):
        b.projection = "cube"                                                      # frozen like the lights
    for wrong in (sky, "sky", (0.2, 0.4, 0.9), Color(0.2, 0.4, 0.9), 1):
        with pytest.raises(TypeError):
            World([], [], wrong)
    for wrong in (None, "plain", Color(0.2, 0.4, 0.9), (sky,)):
        with pytest.raises(TypeError):
            Background(wrong)
    for wrong in ("sphere", "", None, 0, "CUBE"):
        with pytest.raises(ValueError):
            Background(sky, wrong)


def test_rtw_set_background_limits_and_flatten_helpers():
    import raytracer_challenge_amd as rt
    hip = rt.hip_backend()
    assert hip.has_background
    lib = hip.lib
    counts, desc = (C.c_uint32 * 8)(), ff.RtcSceneDesc()
    nw = hip.build_world(floor_world())
    assert lib.rtw_world_flatten_counts(nw.handle, counts) == 0 and counts[7] == 1
    pat = lib.rtw_pattern_plain(0.1, 0.2, 0.3)
    assert lib.rtw_world_set_background(nw.handle, None, BG_DIRECTION) != 0 and "NULL" in hip._err()
    assert lib.rtw_world_set_background(nw.handle, pat, 2) != 0 and "projection of the background" in hip._err()
    assert lib.rtw_world_flatten_counts(nw.handle, counts) == 0                    # a refused call leaves the world as it was
    assert lib.rtw_world_set_background(nw.handle, pat, BG_CUBE) == 0
    assert lib.rtw_world_set_background(nw.handle, pat, BG_DIRECTION) == 0         # a second call replaces the first
    lib.rtw_pattern_release(pat)
    assert lib.rtw_world_flatten_counts(nw.handle, counts) != 0 and "background" in hip._err()
    assert lib.rtw_world_flatten_desc(nw.handle, desc) != 0 and "background" in hip._err()
    nw2 = hip.build_world(floor_world(Background(Pattern.debug(), "cube")))       # ... and through the Python layer
    assert lib.rtw_world_flatten_counts(nw2.handle, counts) != 0 and "background" in hip._err()


# ---- the libraries ----------------------------------------------------------------------------------------------------------------
def test_exports_and_package_names():
    lib = load(LIB)
    for name in ("rtc_scene_create_ext3", "rtc_multi_create_ext3", "rtc_background_point", "rtc_background_colors", "rtc_scene_background_info",
                 "rtw_world_set_background"):
        assert hasattr(lib, name), name
    from raytracer_challenge_amd import scenes
    for skybox in (False, True):
        cam, world = scenes.sky_showcase(32, 18, skybox=skybox)
        assert (cam.hsize, cam.vsize) == (32, 18) and isinstance(world.background, Background)
        assert world.background.projection == ("cube" if skybox else "direction")
        assert world.background.pattern.tag == ("uv" if skybox else "mixture")
        assert any(e.args.material.reflective > 0 and e.args.material.transparency > 0 for e in world.elements)   # a glass ball ...
        assert any(e.args.material.reflective > 0 and e.args.material.transparency == 0 for e in world.elements)  # ... and mirrors


def test_oracle_refuses_a_background(orc):
    assert not orc.has_background
    with pytest.raises(RtwError, match="a background needs librtc_amd.so"):
        orc.build_world(floor_world(Background(Pattern.plain(Color(0.2, 0.4, 0.9)))))
    orc.build_world(floor_world())                                                 # no background: as before


def test_emulator_refuses_a_background():
    """tests/cpu_emu links the product's rtw_capi.cpp without rtc_scene_create_ext3 (the reference to it is weak): the library loads and
    renders worlds without a background; a world with one fails with a message that names it."""
    from emu_lib import emu
    e = emu()
    cam = Camera.new(8, 6, 1.0, Camera.transform(Vector.point(0, 1.5, -5), Vector.point(0, 1, 0), Vector.vector(0, 1, 0)))
    rgb, _ = e.render(e.build_world(World.default()), cam, 1)
    assert np.isfinite(rgb).all() and rgb.max() > 0.0
    nw = e.build_world(floor_world(Background(Pattern.plain(Color(0.2, 0.4, 0.9)))))
    with pytest.raises(RtwError, match="a background needs rtc_scene_create_ext3"):
        e.render(nw, cam, 1)


def test_rust_shim_mirrors_rtc_background():
    h = open(os.path.join(ROOT, "include", "rtc.h")).read()
    rs = open(os.path.join(ROOT, "shim", "gpu.rs")).read()
    c, r = c_struct(h, "rtc_background"), rust_struct(rs, "RtcBackground")
    assert c == r, (c, r)
    assert [f[0] for f in c] == ["pattern", "projection"] and C.sizeof(RtcBackground) == 8
    ci, ri = c_struct(h, "rtc_background_info"), rust_struct(rs, "RtcBackgroundInfo")
    assert ci == ri, (ci, ri)
    assert [f[0] for f in ci] == [f[0] for f in RtcBackgroundInfo._fields_] and C.sizeof(RtcBackgroundInfo) == 40
    for fn in ("rtc_scene_create_ext3", "rtc_multi_create_ext3", "rtc_background_point", "rtc_background_colors", "rtc_scene_background_info"):
        assert "fn %s(" % fn in rs, fn
    assert "RTC_BG_DIRECTION: i32 = 0" in rs and "RTC_BG_CUBE: i32 = 1" in rs
    assert "RTC_BG_DIRECTION = 0, RTC_BG_CUBE = 1" in h


def test_variant_table_is_untouched_and_the_extended_builds_are_its_general_rows():
    """The BG and NP instantiations of the one-kernel path are no rows of RTC_VARIANTS and have no table of their own: the table keeps its
    twelve rows, RtcVariant its five fields, and rtc_feat.hip is built once more per general row of the table and extension."""
    import re
    csrc = os.path.join(ROOT, "raytracer_challenge_amd", "csrc")
    dev = open(os.path.join(csrc, "rtc_device.hpp")).read()
    table = dev[dev.index("constexpr RtcVariant RTC_VARIANTS[] = {"):dev.index("constexpr int RTC_N_VARIANTS")]
    rows = [line.split("//")[0].strip() for line in table.splitlines() if line.strip().startswith("{")]
    assert table.count("},") == 12 and len(rows) == 12 and all(r.count(",") == 5 for r in rows)
    assert re.findall(r"constexpr RtcVariant (\w+)\[", dev) == ["RTC_VARIANTS"]   # one table
    mk = open(os.path.join(csrc, "Makefile")).read()
    assert "VARIANT_IDS := 0 1 2 3 4 5 6 7 8 9 10 11\n" in mk and "GENERAL_IDS := 4 6 8 9 10 11\n" in mk and "EXT_IDS := 1 2 3\n" in mk
    assert [v for v, r in enumerate(rows) if r.startswith("{3, false,")] == [4, 6, 8, 9, 10, 11]   # the general rows, all of them
    # exactly general rows x extensions: one list of units, in OBJS and in the one rule that builds them; no other -D selects a build
    assert "EXT_UNITS := $(foreach v,$(GENERAL_IDS),$(foreach e,$(EXT_IDS),$(v)_ext$(e)))\n" in mk
    assert mk.count("$(foreach x,$(EXT_UNITS),$(O)/rtc_feat$(x).o)") == 2
    assert ("$(foreach x,$(EXT_UNITS),$(O)/rtc_feat$(x).o): $(O)/rtc_feat%.o: rtc_feat.hip $(KHDRS)\n"
            "\t$(HIPCC_C) -DRTC_VARIANT=$(firstword $(subst _ext, ,$*)) -DRTC_EXT=$(lastword $(subst _ext, ,$*)) -c $< -o $@\n") in mk
    assert "$(O)/rtc_feat%.o: rtc_feat.hip $(KHDRS)\n\t$(HIPCC_C) -DRTC_VARIANT=$* -c $< -o $@\n" in mk
    assert set(re.findall(r"-D(RTC_\w+)", mk[mk.index("$(OUT):"):mk.index("resource-usage:")])) == {"RTC_VARIANT", "RTC_EXT"}
    # the feature's own files hold its small kernels and nothing that is compiled in or out
    for name in ("rtc_background.hip", "rtc_bump.hip"):
        assert "#if" not in open(os.path.join(csrc, name)).read(), name
