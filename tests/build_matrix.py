"""The ray kernels' builds, restated, and a table of small scenes each constructed to land on a named build.

The library compiles the ray kernels in several builds (csrc/rtc_device.hpp RTC_VARIANTS, csrc/rtc_feat.hip, csrc/rtc_kernels.hip) and a
chain of host decisions picks the build that renders a scene.  This module restates those rules in Python FROM THE COMMENTS of the table
(nothing is imported from the library), so that the complete set of builds is known to the tests, and lists the scenes that pin each one.
The tests (test_kernel_builds_cpu.py, test_kernel_builds_gpu.py) ask the library which build it would launch (include/rtc.h
rtc_scene_kernel_info) and hold it to this restatement, render every scene under every build it can be switched to, and compare the bits.
"""
import contextlib
import ctypes as C
import math
import os

import numpy as np

from raytracer_challenge_amd.cabi import HIT_DTYPE, RtcCameraC, RtcKernelInfo as KernelInfo, RtcStatsC
from raytracer_challenge_amd.scene import (AreaLight, Camera, Cone, Color, Element, GroupKind, Material, Matrix, Pattern, PointLight, ShapeArgs, SpotLight, Vector, World)

import cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FUEL = 5

# ---- the rules, restated -------------------------------------------------------------------------------------------------------------
# (feat, kops, area, uv, spot) per row.  feat: 0 no gates, 1 whole meshes gated, 2 per-primitive gates, 3 + CSG; kops: the program is read
# from the kernel arguments; area / uv / spot: area lights, UV patterns, light cones.
VARIANTS = (
    (0, True, False, False, False),    # 0
    (1, True, False, False, False),    # 1
    (1, False, False, False, False),   # 2: also serves gate-free programs too long for the kernel arguments
    (2, False, False, False, False),   # 3
    (3, False, False, False, False),   # 4
    (2, True, False, False, False),    # 5: grouped scenes on the fast path
    (3, False, True, False, False),    # 6: serves every scene with an area light that 7 does not
    (1, True, True, False, False),     # 7: area-light scenes variants 0 and 1 would serve
    (3, False, False, True, False),    # 8: the one-kernel path of every scene with a UV pattern
    (3, False, True, True, False),     # 9: the same with an area light
    (3, False, True, False, True),     # 10: every scene with a light cone, area light or not
    (3, False, True, True, True),      # 11: the one-kernel path of a UV scene with a light cone
)
KOPS, KPLANES, KAUX = 12, 6, 3          # ops, plane records and accelerator roots that fit the kernel arguments
LDS_BLOCK, LDS_LIMIT = 768, 158 * 1024  # threads of an LDS-resident traversal block; bytes of tables + stacks that may live in LDS
BIG_SCENE = 32 << 20                    # device bytes above which the one-kernel path takes the 3-waves-per-SIMD build

TRACE = ("default", "count", "lean", "3wave")
WF_TS = ("mem", "mem+count", "lds", "lds+count")
WF_SHADE = ("count", "count+uv", "uv", "pipe+lv0", "pipe", "pat")


def v_wavefront(r): return not r[3]                           # has wf_ts builds
def v_lds(r): return r[1] and not r[2] and not r[3]           # LDS-resident wf_ts builds
def v_trace_3wave(r): return r[0] == 1 and not r[2] and not r[3]
def v_trace_lean(r): return r[0] <= 1 and not r[2] and not r[3]


# Scenes with a background, a bump record or both take, on the one-kernel path, an EXTENSION of a general row: feature level 3, program read
# from memory, the scene's own area / uv / spot flags ("a cone always comes with the `area` code path").  The library builds every general
# row once more per extension and reports the build by number (include/rtc.h rtc_background_info / rtc_bump_info .trace_build).
EXTENSIONS = ("none", "bg", "np", "np+bg")                    # RtcExt 0..3
def v_general(r): return r[0] == 3 and not r[1]


def general_row(area, uv, spot):
    """The one general row that serves a scene's flags."""
    rows = [v for v, r in enumerate(VARIANTS) if v_general(r) and r[2:] == (area or spot, uv, spot)]
    assert len(rows) == 1, (area, uv, spot, rows)
    return rows[0]


def ext_build(area, uv, spot, bg):
    """The number reported: "0 none, 1 area, 2 uv, 3 area + uv, 4 spot, 5 spot + uv -- and for a bumped scene with a background 6 more"."""
    return ((5 if uv else 4) if spot else (2 if uv else 0) + (1 if area else 0)) + (6 if bg else 0)


def pick_variant(feat, kops, area, uv, spot, wavefront):
    if spot:
        return 11 if (uv and not wavefront) else 10            # wider light records: no other variant can read them
    if uv and not wavefront:
        return 9 if area else 8                                # (the wavefront path of a UV scene: only wf_shade differs)
    if area:
        return 7 if (feat <= 1 and kops) else 6
    if feat <= 1 and kops:
        return feat
    if feat == 2 and kops:
        return 5
    return 2 if feat <= 1 else feat + 1


def trace_build(row, count, big, all_plain, no_glass_mirror):
    r = VARIANTS[row]
    if v_trace_3wave(r) and big and not count:
        return "3wave"
    if v_trace_lean(r) and not count and all_plain and no_glass_mirror:
        return "lean"
    return "count" if count else "default"


def wf_ts_build(count, lds): return ("lds" if lds else "mem") + ("+count" if count else "")


def wf_shade_build(count, uv, all_plain, level0):
    if uv:
        return "count+uv" if count else "uv"
    if count:
        return "count"
    if all_plain:
        return "pipe+lv0" if level0 else "pipe"
    return "pat"


def lds_table_bytes(n_bvh, n_recs, n_mtri, has_recs, has_mesh):
    """7 rows of 16 B per node; 8 rows of 16 B per record if a program op reads records; 9 doubles + one int per mesh triangle, padded to 16."""
    b = 7 * 16 * n_bvh
    if has_recs:
        b += 8 * 16 * n_recs
    if has_mesh:
        b += (76 * n_mtri + 15) & ~15
    return b


def lds_bytes(row, enabled, table_bytes, bvh_stack):
    if not enabled or not v_lds(VARIANTS[row]):
        return 0
    need = table_bytes + LDS_BLOCK * bvh_stack * 4
    return need if need <= LDS_LIMIT else 0


def all_builds(rows=range(len(VARIANTS)), counts=(False, True), lds=True, uv=True):
    """Every (row, kernel, build) the library holds for `rows`; wf_shade is one kernel for all rows (row None), level 0 apart."""
    out = set()
    for v in rows:
        r = VARIANTS[v]
        for c in counts:
            out.add((v, "trace", "count" if c else "default"))
            if v_wavefront(r):
                out.add((v, "wf_ts", wf_ts_build(c, False)))
                if lds and v_lds(r):
                    out.add((v, "wf_ts", wf_ts_build(c, True)))
        if False in counts:
            if v_trace_lean(r):
                out.add((v, "trace", "lean"))
            if v_trace_3wave(r):
                out.add((v, "trace", "3wave"))
    for c in counts:
        for u in ((False, True) if uv else (False,)):
            for plain in (False, True):
                out.add((None, "wf_shade0", wf_shade_build(c, u, plain, True)))
                out.add((None, "wf_shade", wf_shade_build(c, u, plain, False)))
    return out


# ---- the switches ----------------------------------------------------------------------------------------------------------------------
# Environment variables read when a scene is created; each sends a scene to another build that must compute the same bits.
SWITCHES = {"default": {}, "no_kops": {"RTC_NO_KOPS": "1"}, "no_kops_groups": {"RTC_KOPS_GROUPS": "0"}, "no_lds": {"RTC_WF_LDS": "0"}}


@contextlib.contextmanager
def environment(**kw):
    """os.environ with `kw` set (None: unset) for the block."""
    old = {k: os.environ.get(k) for k in kw}
    try:
        for k, v in kw.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
        yield
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def switched(switch, path):
    env = {"RTC_NO_KOPS": None, "RTC_KOPS_GROUPS": None, "RTC_WF_LDS": None, "RTC_KERNEL": str(path)}
    env.update(SWITCHES[switch])
    return environment(**env)


class Facts:
    """What the dispatch reads of a scene, as the table states it (not read back from the library)."""

    def __init__(self, feat, fits, area=False, uv=False, spot=False, all_plain=False, no_glass_mirror=True, big=False, lds=False):
        self.feat, self.fits, self.area, self.uv, self.spot = feat, fits, area, uv, spot
        self.all_plain, self.no_glass_mirror, self.big, self.lds = all_plain, no_glass_mirror, big, lds

    def predict(self, switch, path, count, emulator=False):
        """{variant, kops, lds, trace | wf_ts, wf_shade0, wf_shade} of a launch under `switch`.  The emulator has no LDS-resident build
        and never calls a scene big."""
        kops = self.fits and switch != "no_kops" and not (switch == "no_kops_groups" and self.feat == 2) and self.feat < 3
        wavefront = path == 4
        row = pick_variant(self.feat, kops, self.area, self.uv, self.spot, wavefront)
        out = {"variant": row, "kops": kops}
        if wavefront:
            lds = self.lds and kops and switch != "no_lds" and v_lds(VARIANTS[row]) and not emulator
            out.update(lds=lds, wf_ts=wf_ts_build(count, lds), wf_shade0=wf_shade_build(count, self.uv, self.all_plain, True),
                       wf_shade=wf_shade_build(count, self.uv, self.all_plain, False))
        else:
            out.update(lds=False, trace=trace_build(row, count, self.big and not emulator, self.all_plain, self.no_glass_mirror))
        return out

    def changes(self, switch, emulator=False):
        """Does `switch` send some launch of the scene to another build than the default?"""
        return any(self.predict(switch, p, c, emulator) != self.predict("default", p, c, emulator) for p in (1, 4) for c in (False, True))


# ---- the hook ---------------------------------------------------------------------------------------------------------------------------
def reported(self, path):
    """The same record Facts.predict gives, from an rtc_kernel_info (`self`)."""
    out = {"variant": self.variant, "kops": self.n_kops > 0, "lds": self.lds_bytes > 0}
    if path == 4:
        assert self.trace_build == -1
        out.update(wf_ts=WF_TS[self.wf_ts_build], wf_shade0=WF_SHADE[self.wf_shade_build0], wf_shade=WF_SHADE[self.wf_shade_build])
    else:
        assert self.wf_ts_build == self.wf_shade_build0 == self.wf_shade_build == -1 and self.lds_bytes == 0
        out.update(trace=TRACE[self.trace_build])
    return out


def scene_of(backend, nw, device=0):
    scene = backend.lib.rtw_world_scene(nw.handle, device)
    assert scene, backend._err()
    return scene


def kernel_info(backend, nw, path, count, device=0):
    k = KernelInfo()
    assert backend.lib.rtc_scene_kernel_info(scene_of(backend, nw, device), path, 1 if count else 0, C.byref(k)) == 0, backend.lib.rtc_last_error()
    return k


def n_ops(backend, nw):
    a = [C.c_uint32(0) for _ in range(4)]
    backend.lib.rtc_scene_accel_info(scene_of(backend, nw), *[C.byref(x) for x in a])
    return a[0].value


def ledger_items(info, path):
    """The (row, kernel, build) triples a launch with this report runs."""
    r = reported(info, path)
    if path == 1:
        return {(r["variant"], "trace", r["trace"])}
    return {(r["variant"], "wf_ts", r["wf_ts"]), (None, "wf_shade0", r["wf_shade0"]), (None, "wf_shade", r["wf_shade"])}


# ---- scenes ---------------------------------------------------------------------------------------------------------------------------
def plain(r, g, b, **kw):
    return Material(pattern=Pattern.plain(Color.new(r, g, b)), **kw)


GLASS_MIRROR = dict(diffuse=0.2, transparency=0.8, reflective=0.4, refractive_index=1.5)


def camera(frm=(0.5, 1.2, -5.5), to=(0.0, 0.6, 0.0), fov=1.1, h=48, v=32):
    return Camera.new(h, v, fov, Camera.transform(Vector.point(*frm), Vector.point(*to), Vector.vector(0, 1, 0)))


LIGHTS = [PointLight(Color.white(), Vector.point(-4.0, 6.5, -5.0)), PointLight(Color.new(0.3, 0.3, 0.45), Vector.point(5.0, 4.0, -3.0))]


def room_planes(n, last=None):
    """n planes around the origin, all facing it: floor, back wall, side walls, ceiling, front wall, then slanted ones that cut the
    room's corners in view of the camera.  Plane k's material is mirror-like on every third one.  `last`: the material of plane n - 1."""
    spec = [(0.0, 0.0, 1.0), (0.0, -math.pi / 2, 6.0), (math.pi / 2, -math.pi / 2, 7.0), (-math.pi / 2, -math.pi / 2, 7.0), (0.0, math.pi, 8.0),
            (0.0, math.pi / 2, 9.0), (0.6, -1.1, 5.0), (-0.6, -1.1, 5.0), (0.3, -2.2, 6.0), (-0.3, -2.2, 6.0), (1.2, -0.7, 5.5), (-1.2, -0.7, 5.5),
            (0.9, -1.9, 6.5)]
    out = []
    for k in range(n):
        ry, rx, d = spec[k]
        t = Matrix.rotation_y(ry) * Matrix.rotation_x(rx) * Matrix.translation(0.0, -d, 0.0)
        m = plain(0.35 + 0.05 * (k % 7), 0.75 - 0.04 * k, 0.4 + 0.04 * k, reflective=0.3 if k % 3 == 0 else 0.0, specular=0.2)
        out.append(Element.plane(ShapeArgs(transform=t, material=last if (last is not None and k == n - 1) else m)))
    return out


def balls(n=6, glass_mirror=False, pattern=None):
    """n spheres and closed cylinders on a ring above the floor (6 or more become one analytic BVH)."""
    out = []
    for i in range(n):
        a = 2.0 * math.pi * i / n + 0.3
        t = Matrix.translation(1.9 * math.cos(a), 0.1 + 0.35 * (i % 3), 1.4 * math.sin(a)) * Matrix.scaling(0.55, 0.55, 0.55)
        m = plain(0.9 - 0.1 * i, 0.2 + 0.1 * i, 0.3, reflective=0.5 if i % 2 else 0.0, transparency=0.6 if i == 4 else 0.0, refractive_index=1.3)
        if glass_mirror and i == 0:
            m = plain(0.1, 0.1, 0.15, **GLASS_MIRROR)
        if pattern is not None and i == 2:
            m = Material(pattern=pattern, specular=0.3)
        args = ShapeArgs(transform=t, material=m)
        out.append(Element.cylinder(args, -0.8, 0.9, True) if i % 4 == 3 else Element.sphere(args))
    return out


def program_scene(n_planes, gated=False, glass_mirror=False):
    """n_planes + 1 ops: the planes and one analytic BVH of six shapes.  All materials Plain; no material both reflects and refracts
    unless glass_mirror.  gated: the six shapes sit in a transformed aggregation group (per-primitive gates: feature level 2)."""
    shapes = balls(6, glass_mirror)
    if gated:
        shapes = [Element.composite(Matrix.translation(0.0, 0.05, 0.1) * Matrix.rotation_y(0.2), None, GroupKind.Aggregation, shapes)]
    return camera(), World(LIGHTS, room_planes(n_planes) + shapes)


TEAPOT = os.path.join(ROOT, "assets", "obj", "teapot_low.obj")


def teapot(x, y, z, s, ry, mat):
    return Element.obj(TEAPOT, Matrix.translation(x, y, z) * Matrix.rotation_y(ry) * Matrix.rotation_x(-math.pi / 2) * Matrix.scaling(s, s, s), mat)


def plane_edge_scene(n_planes):
    """n_planes planes and one mesh: no op but a plane beyond the sixth reads the record table.  The LAST plane stands between the first
    light and the teapot, slanted, and is transparent (it casts a shadow all the same): camera rays pass through it, so it is the first
    hit of the pixels in front of the teapot and the shadow blocker of everything seen behind it."""
    veil = plain(0.6, 0.7, 0.9, diffuse=0.3, transparency=0.85, refractive_index=1.0)
    planes = room_planes(n_planes - 1)
    last = Element.plane(ShapeArgs(transform=Matrix.translation(-1.6, 2.6, -2.2) * Matrix.rotation_z(-0.85) * Matrix.rotation_x(0.55), material=veil))
    return camera(), World(LIGHTS, planes + [last, teapot(0.2, 0.0, 0.3, 0.12, 0.5, plain(0.85, 0.6, 0.3, specular=0.4))])


def aux_scene(n_meshes, with_bvh=False):
    """n_meshes transformed copies of the low teapot (one accelerator op each) over two planes; with_bvh: and an analytic BVH of six
    shapes, which the program lists after the meshes.  The LAST accelerator stands nearest to the camera and to the first light: the
    closest hit of the pixels on it and the shadow blocker of the others behind it."""
    spots = [(-1.9, 0.0, 1.8, 0.10, 0.3), (1.9, 0.0, 1.8, 0.10, -0.4), (0.0, 0.0, 2.6, 0.12, 0.0), (-0.7, 0.0, -1.2, 0.11, 0.8)]
    els = room_planes(2)
    for i in range(n_meshes):
        x, y, z, s, ry = spots[i] if not with_bvh or i < 3 else spots[3]
        els.append(teapot(x, y, z, s, ry, plain(0.3 + 0.2 * i, 0.8 - 0.15 * i, 0.5, reflective=0.2 if i == 1 else 0.0, specular=0.5)))
    if with_bvh:
        els += [Element.composite(Matrix.translation(-0.6, 0.3, -1.6) * Matrix.scaling(0.45, 0.45, 0.45), None, GroupKind.Aggregation, [])]  # (an empty group: no op)
        els += [Element.sphere(ShapeArgs(transform=Matrix.translation(-0.9 + 0.35 * i, 0.35 + 0.2 * (i % 2), -1.5 + 0.1 * i) * Matrix.scaling(0.3, 0.3, 0.3),
                                         material=plain(0.9, 0.3 + 0.1 * i, 0.2, **(GLASS_MIRROR if i == 4 else {})))) for i in range(6)]
    return camera(), World(LIGHTS, els)


def write_grid_obj(path, nx, nz, n_faces=None, seed=3):
    """A small displaced grid as one OBJ group of flat triangles, the first n_faces of its 2 (nx - 1)(nz - 1) only: any triangle count."""
    rng = np.random.default_rng(seed)
    xs, zs = np.linspace(-1.0, 1.0, nx), np.linspace(-1.0, 1.0, nz)
    with open(path, "w") as f:
        f.write("g Grid\n")
        for z in zs:
            for x in xs:
                f.write("v %.17g %.17g %.17g\n" % (x, 0.25 * math.sin(3.0 * x + 0.5) * math.cos(2.5 * z) + 0.02 * rng.uniform(-1, 1), z))
        faces = []
        for j in range(nz - 1):
            for i in range(nx - 1):
                a = j * nx + i + 1
                faces += [(a, a + nx, a + 1), (a + 1, a + nx, a + nx + 1)]
        for a, b, c in faces[:n_faces]:
            f.write("f %d %d %d\n" % (a, b, c))
    return len(faces[:n_faces])


def grid_scene(path, n_planes=2, with_bvh=False):
    """The grid mesh of `path` above n_planes planes (a mesh-only scene reads no records); with_bvh: and an analytic BVH of six shapes."""
    mesh = Element.obj(path, Matrix.translation(0.0, 0.7, 0.4) * Matrix.rotation_x(-0.5) * Matrix.scaling(1.8, 1.0, 1.4), plain(0.3, 0.7, 0.9, reflective=0.2, specular=0.4))
    return camera(), World(LIGHTS, room_planes(n_planes) + [mesh] + (balls(6) if with_bvh else []))


def area_world(world, degenerate=False):
    """Every light of `world` as a 2x2 area light of 1x1 units around it, or (degenerate) with all four samples at the light's origin: the
    latter renders exactly the point-light world, which the oracle knows."""
    P, V = Vector.point, Vector.vector
    z = V(0.0, 0.0, 0.0)
    if degenerate:
        return World([AreaLight(l.intensity, l.origin, z, 2, z, 2) for l in world.lights], world.elements)
    return World([AreaLight(l.intensity, P(l.origin[0] - 0.5, l.origin[1], l.origin[2] - 0.5), V(1.0, 0.0, 0.0), 2, V(0.0, 0.0, 1.0), 2) for l in world.lights], world.elements)


def open_cones(world):
    """Every point light with a cone of half-angle pi (cos = -1: full everywhere): the spot code paths, the no-cone world's pixels."""
    out = []
    for l in world.lights:
        if isinstance(l, AreaLight):
            out.append(AreaLight(l.intensity, l.corner, l.uvec, l.usteps, l.vvec, l.vsteps, l.jitter, cone=Cone(Vector.vector(0, -1, 0), math.pi, math.pi)))
        else:
            out.append(SpotLight(l.intensity, l.origin, Vector.vector(0.0, -1.0, 0.0), math.pi, math.pi))
    return World(out, world.elements)


def real_cones(world):
    """Every light with a cone aimed at the scene's middle, full within 0.25 rad and dark beyond 0.45: pixels in the light, in the smooth
    band and in the dark.  No reference scene equals it: compared build against build only."""
    out = []
    for l in world.lights:
        o = l.corner if isinstance(l, AreaLight) else l.origin
        axis = Vector.vector(0.3 - o[0], 0.2 - o[1], 0.2 - o[2])
        if isinstance(l, AreaLight):
            out.append(AreaLight(l.intensity, l.corner, l.uvec, l.usteps, l.vvec, l.vsteps, l.jitter, cone=Cone(axis, 0.25, 0.45)))
        else:
            out.append(SpotLight(l.intensity, l.origin, axis, 0.25, 0.45))
    return World(out, world.elements)


UV_COLOR = Color.new(0.2, 0.55, 0.85)


def uv_pattern(two_colours=False):
    """Spherical UV checkers whose two colours are the same Plain colour: the UV code paths, a Plain(UV_COLOR) material's pixels.
    two_colours: real checkers, whose pixels depend on the (u, v) computed."""
    from raytracer_challenge_amd.texture import UvPattern
    other = Pattern.plain(Color.new(0.95, 0.9, 0.2)) if two_colours else Pattern.plain(UV_COLOR)
    return Pattern.texture_map(Matrix.rotation_y(0.3), "spherical", UvPattern.checkers(8.0, 4.0, Pattern.plain(UV_COLOR), other))


def small_world(uv=False, csg=False):
    """Two planes and six shapes, one of them glass-and-mirror; uv: one with a UV pattern (Plain(UV_COLOR) for the oracle; "real": checkers
    of two colours); csg: and a carved cube."""
    els = room_planes(2) + balls(6, glass_mirror=True, pattern=uv_pattern(uv == "real") if uv else Pattern.plain(UV_COLOR))
    if csg:
        els.append(Element.composite(Matrix.translation(0.0, 0.4, -1.0) * Matrix.rotation_y(0.5) * Matrix.scaling(0.5, 0.5, 0.5), None, GroupKind.Difference, [
            Element.cube(ShapeArgs(material=plain(0.9, 0.7, 0.2))), Element.sphere(ShapeArgs(transform=Matrix.scaling(1.3, 1.3, 1.3), material=plain(0.8, 0.1, 0.1, reflective=0.3)))]))
    return camera(), World(LIGHTS, els)


class Entry:
    """One scene of the table.  make(tmp) -> (camera, world); oracle(world) -> the world the oracle renders instead (a scene with an
    extension the reference has not, built so that it equals a reference scene); facts: what the dispatch reads of it; rows: the row on
    the one-kernel and on the wavefront path; pins: what the entry is in the table for.  oracle=False: no reference scene equals it, its
    builds are compared with each other only.  hit=(lo, hi): some camera ray and some explicit ray must have its closest hit on a
    primitive lo <= p < hi (what the scene is aimed at)."""

    def __init__(self, name, make, facts, rows, pins, oracle=None, n_ops=None, emulated=True, check=None, hit=None):
        self.name, self.make, self.facts, self.rows, self.pins = name, make, facts, rows, pins
        self.oracle_link = oracle is not False
        self.oracle = oracle or ((lambda w: World(LIGHTS, w.elements)) if oracle is False else (lambda w: w))   # (also the world the rays are aimed at)
        self.n_ops, self.emulated, self.check, self.hit = n_ops, emulated, check, hit

    def __repr__(self):
        return self.name


def _grid(tmp, nx, nz, n_faces=None):
    path = os.path.join(str(tmp), "grid_%dx%d_%s.obj" % (nx, nz, n_faces))
    if not os.path.exists(path):
        write_grid_obj(path, nx, nz, n_faces)
    return path


def _with(world_fn, f):
    def make(tmp):
        cam, world = world_fn(tmp)
        return cam, f(world)
    return make


def _is(**want):
    def check(info):
        for k, v in want.items():
            assert getattr(info, k) == v, "%s = %d, the table says %d" % (k, getattr(info, k), v)
    return check


F = Facts
TABLE = [
    # program-length edges: exactly RTC_KOPS ops, and one more
    Entry("ops12", lambda tmp: program_scene(11), F(0, True, all_plain=True, lds=True), (0, 0), "row 0: LEAN, LDS tables with an analytic BVH and no mesh; 12 ops",
          n_ops=12, check=_is(n_kops=12, n_kplanes=6, n_kaux=1, has_recs=1, has_mesh=0)),
    Entry("ops13", lambda tmp: program_scene(12), F(0, False, all_plain=True), (2, 2), "row 2: a gate-free program one op too long; LEAN of row 2", n_ops=13, check=_is(n_kops=0)),
    Entry("ops12_gated", lambda tmp: program_scene(11, gated=True), F(2, True, all_plain=True, lds=True), (5, 5), "row 5; 12 ops with per-primitive gates", n_ops=12,
          check=_is(n_kops=12)),
    Entry("ops13_gated", lambda tmp: program_scene(12, gated=True), F(2, False, all_plain=True), (3, 3), "row 3: a gated program one op too long", n_ops=13, check=_is(n_kops=0)),
    Entry("ops12_glass_mirror", lambda tmp: program_scene(11, glass_mirror=True), F(0, True, all_plain=True, no_glass_mirror=False, lds=True), (0, 0),
          "row 0 default build: one glass-mirror material leaves LEAN", n_ops=12, check=_is(all_plain=1, no_glass_mirror=0)),
    # plane edge: RTC_KPLANES plane records, and one more
    Entry("planes6", lambda tmp: plane_edge_scene(6), F(1, True, all_plain=True, lds=True), (1, 1), "row 1: LEAN; LDS tables of a mesh-only scene that reads no records",
          check=_is(n_kplanes=6, has_recs=0, has_mesh=1, n_kaux=1)),
    Entry("planes7", lambda tmp: plane_edge_scene(7), F(1, True, all_plain=True, lds=True), (1, 1), "the 7th plane falls out of the kernel arguments into the record table",
          check=_is(n_kplanes=6, has_recs=1, has_mesh=1), hit=(6, 7)),
    # aux edge: RTC_KAUX accelerator roots, and one more
    Entry("aux3", lambda tmp: aux_scene(3), F(1, True, all_plain=True, lds=True), (1, 1), "three accelerator roots in the kernel arguments", check=_is(n_kaux=3, n_kops=5)),
    Entry("aux4", lambda tmp: aux_scene(4), F(1, True, all_plain=True, lds=True), (1, 1), "the 4th mesh reads its root and frame from memory", check=_is(n_kaux=3, n_kops=6),
          hit=(2 + 3 * 240, 2 + 4 * 240)),
    Entry("aux4_bvh", lambda tmp: aux_scene(3, with_bvh=True), F(1, True, all_plain=True, no_glass_mirror=False), (1, 1),
          "the analytic BVH is the 4th accelerator; row 1 default build; one record per triangle: too many for LDS",
          check=_is(n_kaux=3, n_kops=6, has_recs=1, has_mesh=1), hit=(2 + 3 * 240, 2 + 3 * 240 + 6)),
    # LDS layout edges (the counts are asserted by the GPU tests from the hook's own figures)
    Entry("grid_mesh", lambda tmp: grid_scene(_grid(tmp, 6, 4)), F(1, True, all_plain=True, lds=True), (1, 1), "LDS triangle table whose 76 B records do not fill 16 B units",
          check=_is(has_recs=0, has_mesh=1)),
    Entry("grid_mesh_bvh", lambda tmp: grid_scene(_grid(tmp, 8, 4), with_bvh=True), F(1, True, all_plain=True, lds=True), (1, 1), "LDS nodes, records and triangles together",
          check=_is(has_recs=1, has_mesh=1)),
    # the other rows
    Entry("csg", lambda tmp: small_world(csg=True), F(3, False, no_glass_mirror=False, all_plain=True), (4, 4), "row 4"),
    Entry("patterned", lambda tmp: cases.pattern_world(cases.nested_pattern("checkers", 2)), F(0, True, lds=True), (0, 0), "wf_shade PAT build; row 0 default build"),
    Entry("area_kops", _with(lambda tmp: small_world(), lambda w: area_world(w, True)), F(0, True, area=True, all_plain=True, no_glass_mirror=False), (7, 7), "row 7: kops plus area",
          oracle=lambda w: World(LIGHTS, w.elements), emulated=False),
    Entry("area_csg", _with(lambda tmp: small_world(csg=True), lambda w: area_world(w, True)), F(3, False, area=True, all_plain=True, no_glass_mirror=False), (6, 6), "row 6",
          oracle=lambda w: World(LIGHTS, w.elements), emulated=False),
    Entry("uv", lambda tmp: small_world(uv=True), F(0, True, uv=True, no_glass_mirror=False, lds=True), (8, 0), "row 8; wf_shade UV builds", emulated=False,
          oracle=lambda w: small_world(uv=False)[1]),
    Entry("uv_area", _with(lambda tmp: small_world(uv=True), lambda w: area_world(w, True)), F(0, True, uv=True, area=True, no_glass_mirror=False), (9, 7), "row 9", emulated=False,
          oracle=lambda w: small_world(uv=False)[1]),
    Entry("spot", _with(lambda tmp: small_world(), open_cones), F(0, True, spot=True, all_plain=True, no_glass_mirror=False), (10, 10), "row 10: a cone on point lights", emulated=False,
          oracle=lambda w: World(LIGHTS, w.elements)),
    Entry("spot_area", _with(lambda tmp: small_world(), lambda w: open_cones(area_world(w, True))), F(0, True, spot=True, area=True, all_plain=True, no_glass_mirror=False), (10, 10),
          "row 10: a cone on area lights", emulated=False, oracle=lambda w: World(LIGHTS, w.elements)),
    Entry("uv_spot", _with(lambda tmp: small_world(uv=True), open_cones), F(0, True, uv=True, spot=True, no_glass_mirror=False), (11, 10), "row 11", emulated=False,
          oracle=lambda w: small_world(uv=False)[1]),
    # rows 6..11 again with lights and patterns that are no identity: real penumbrae, a real cone, checkers of two colours.  No reference
    # scene equals them, so they carry no oracle link: their builds are compared with each other.
    Entry("area_kops_real", _with(lambda tmp: small_world(), area_world), F(0, True, area=True, all_plain=True, no_glass_mirror=False), (7, 7), "row 7, 2x2 samples apart",
          oracle=False, emulated=False),
    Entry("area_csg_real", _with(lambda tmp: small_world(csg=True), area_world), F(3, False, area=True, all_plain=True, no_glass_mirror=False), (6, 6), "row 6, 2x2 samples apart",
          oracle=False, emulated=False),
    Entry("uv_real", lambda tmp: small_world(uv="real"), F(0, True, uv=True, no_glass_mirror=False, lds=True), (8, 0), "row 8 and wf_shade UV, checkers of two colours",
          oracle=False, emulated=False),
    Entry("uv_area_real", _with(lambda tmp: small_world(uv="real"), area_world), F(0, True, uv=True, area=True, no_glass_mirror=False), (9, 7), "row 9, the same with penumbrae",
          oracle=False, emulated=False),
    Entry("spot_real", _with(lambda tmp: small_world(), lambda w: real_cones(World([w.lights[0], area_world(w).lights[1]], w.elements))),
          F(0, True, spot=True, area=True, all_plain=True, no_glass_mirror=False), (10, 10), "row 10, a smooth-edged cone on a point and on an area light", oracle=False, emulated=False),
    Entry("uv_spot_real", _with(lambda tmp: small_world(uv="real"), real_cones), F(0, True, uv=True, spot=True, no_glass_mirror=False), (11, 10), "row 11, cone and checkers",
          oracle=False, emulated=False),
]
BY_NAME = {e.name: e for e in TABLE}


def rays_for(world, n=1024):
    """Explicit rays of an entry (they take another pixel-map mode than a camera's): the shared edge rays and rays aimed at the scene's
    own special points."""
    return np.concatenate([cases.edge_rays(n), cases.special_rays(world, n)])


def panic_free(orc, world, rays, fuel=FUEL):
    """Mask of the rays the reference does not panic on (parity.assert_ray_parity_with_panics finds them the same way).  `orc` may be the
    device back end instead, which refuses the same rays with RTC_ERR_NAN: where the oracle is too slow for the whole set."""
    nw = orc.build_world(world)
    keep = np.ones(len(rays), dtype=bool)

    def raises(lo, hi):
        try:
            orc.color_at(nw, rays[lo:hi], fuel)
            return False
        except Exception as ex:  # noqa: BLE001
            if "NaN" not in str(ex):
                raise
            return True

    def find(lo, hi):
        if not raises(lo, hi):
            return
        if hi - lo == 1:
            keep[lo] = False
            return
        mid = (lo + hi) // 2
        find(lo, mid)
        find(mid, hi)

    find(0, len(rays))
    return keep


# ---- rendering one entry under every build -------------------------------------------------------------------------------------------
def render_with_stats(backend, nw, cam, fuel=FUEL):
    """rtc_render with a stats pointer (the counting builds): (rgb, hits)."""
    lib = backend.lib
    cc, rc = backend.camera_c(cam), RtcCameraC()
    assert lib.rtw_make_camera(C.byref(cc), C.byref(rc)) == 0
    n = cam.hsize * cam.vsize
    rgb, hits, st = np.empty((n, 3)), np.empty(n, dtype=HIT_DTYPE), RtcStatsC()
    assert lib.rtc_render(scene_of(backend, nw), C.byref(rc), fuel, None, 0, n, rgb.ctypes.data, hits.ctypes.data, C.byref(st)) == 0, lib.rtc_last_error()
    assert st.rays_primary == n
    return rgb, hits


def frames_of(backend, nw, cam, rays, fuel=FUEL):
    """Everything one scene object renders: the frame without and with counters, its hit-tree digests, the explicit rays."""
    rgb, hits = backend.render(nw, cam, fuel)
    crgb, chits = render_with_stats(backend, nw, cam, fuel)
    dig = backend.render_digest(nw, cam, fuel)
    rrgb, rhits = backend.color_at(nw, rays, fuel)
    return {"rgb": rgb, "hits": hits, "rgb (stats)": crgb, "hits (stats)": chits, "digest": dig, "ray rgb": rrgb, "ray hits": rhits}


def same_bits(a, b, what):
    for k in a:
        x, y = np.ascontiguousarray(a[k]), np.ascontiguousarray(b[k])
        assert x.shape == y.shape and x.tobytes() == y.tobytes(), "%s: %s differs in %d of %d elements" % (
            what, k, int((x.view(np.uint8).reshape(len(x), -1) != y.view(np.uint8).reshape(len(y), -1)).any(axis=1).sum()), len(x))
    assert np.array_equal(a["rgb"].view(np.uint64), a["rgb (stats)"].view(np.uint64)) and a["hits"].tobytes() == a["hits (stats)"].tobytes(), \
        "%s: the counting builds render another frame than the plain ones" % what


def check_hook(backend, entry, world, switch, emulator, ledger=None):
    """The hook's report of `world` under `switch` against the restatement, for both paths with and without counters.  Returns whether
    the switch changed a build, as the hook reports it."""
    changed, base = False, {}
    if switch != "default":
        with switched("default", 1):
            nw = backend.build_world(world)
            base = {(p, c): reported(kernel_info(backend, nw, p, c), p) for p in (1, 4) for c in (False, True)}
            nw.close()
    with switched(switch, 1):
        nw = backend.build_world(world)
        for path in (1, 4):
            for count in (False, True):
                info = kernel_info(backend, nw, path, count)
                got, want = reported(info, path), entry.facts.predict(switch, path, count, emulator)
                assert got == want, "%s under %s, path %d, count %d: the library reports %s, the table says %s" % (entry.name, switch, path, count, got, want)
                assert (info.all_plain, info.no_glass_mirror) == (int(entry.facts.all_plain), int(entry.facts.no_glass_mirror)), entry.name
                assert info.big_scene == int(entry.facts.big and not emulator), entry.name
                if ledger is not None:
                    ledger |= ledger_items(info, path)
                if switch == "default":
                    assert info.variant == entry.rows[0 if path == 1 else 1], "%s: row %d on path %d, the table names %d" % (entry.name, info.variant, path, entry.rows[path != 1])
                    if entry.n_ops is not None:
                        assert n_ops(backend, nw) == entry.n_ops, "%s: %d ops, built for %d" % (entry.name, n_ops(backend, nw), entry.n_ops)
                    if entry.check:
                        entry.check(info)
                else:
                    changed = changed or base[(path, count)] != got
        nw.close()
    return changed


def one_answer(backend, orc, entry, tmp, emulator, paths=(1, 4), oracle_pixels=None, oracle_rays=None):
    """Assertions 2 and 3 for one entry: the oracle link on the default build, then every build the entry can be switched to against the
    default frame, bit for bit: the whole frame and all 2 048 explicit rays.  Returns the (entry, switch) pairs skipped because the switch
    changes nothing.  oracle_pixels / oracle_rays: what the oracle renders where it is too slow for everything (default: the frame and
    every ray); the rays it would panic on are then found by the device's own refusal."""
    from parity import RGB_TOL, assert_parity, assert_ray_parity_with_panics, oracle_reference, rgb_error
    cam, world = entry.make(tmp)
    ref_world = entry.oracle(world)
    rays = rays_for(ref_world)
    with switched("default", paths[0]):
        if entry.oracle_link and oracle_rays is None:
            keep = panic_free(orc, ref_world, rays)
        else:
            keep = panic_free(backend, world, rays)
        # 3. the oracle link, with the existing checks and tolerances
        if entry.oracle_link:
            assert_parity(backend, orc, world, cam, FUEL, oracle_pixels, label=entry.name, ref=oracle_reference(orc, ref_world, cam, FUEL, oracle_pixels))
            some = rays if oracle_rays is None else rays[::len(rays) // oracle_rays][:oracle_rays]
            if ref_world is world:
                assert_ray_parity_with_panics(backend, orc, world, some, FUEL, label=entry.name + " rays")
            else:  # (a world with lights or patterns the oracle has not: the same comparison against the oracle's equivalent world)
                nw = backend.build_world(world)
                rgb, hits = backend.color_at(nw, rays[keep], FUEL)
                nw.close()
                ref_rgb, ref_hits = orc.color_at(orc.build_world(ref_world), rays[keep], FUEL)
                assert hits.tobytes() == ref_hits.tobytes(), entry.name + " rays: hit records differ"
                assert rgb_error(rgb, ref_rgb, entry.name + " rays") <= RGB_TOL
    # 2. one answer per scene
    rays = rays[keep]
    base, skipped = None, []
    for switch in SWITCHES:
        if switch != "default":
            changed = check_hook(backend, entry, world, switch, emulator)
            assert changed == entry.facts.changes(switch, emulator), "%s: switch %s %s a build, the table says otherwise" % (entry.name, switch, "changes" if changed else "does not change")
            if not changed:
                skipped.append((entry.name, switch))
                continue
        for path in paths:
            with switched(switch, path):
                nw = backend.build_world(world)
                got = frames_of(backend, nw, cam, rays)
                if path == 4:  # (the one choice made at launch time: a device that refuses the LDS size runs the memory build)
                    assert kernel_info(backend, nw, 4, False).lds_refused == 0, "%s: the device refused the dynamic LDS size" % entry.name
                nw.close()
            if base is None:
                base = got
                if entry.hit is not None:  # the scene is still aimed at what it is in the table for
                    for k in ("hits", "ray hits"):
                        assert ((got[k]["prim"] >= entry.hit[0]) & (got[k]["prim"] < entry.hit[1])).any(), "%s: no closest hit of %s on primitives %s" % (entry.name, k, entry.hit)
            same_bits(got, base, "%s under %s on path %d against the default build on path %d" % (entry.name, switch, path, paths[0]))
    return skipped


def predicted_skips(entries, emulator):
    return sorted((e.name, s) for e in entries for s in SWITCHES if s != "default" and not e.facts.changes(s, emulator))
