"""Cases shared by test_wf_ts_round_trips_cpu.py (the emulated kernels) and test_wf_ts_round_trips_gpu.py: the three places where the
traversal kernel of the wavefront path (wf_ts) reads memory on its own account, not for a ray --

  the chunk cursor: frames of 8x8, 56x8, 64x8 and 72x8 pixels are 1, 7, 8 and 9 chunks of level 0 (64 work
  ids each: 8x8 tiles) -- below, at and above the eight cursor residues, and far fewer chunks than waves, so most waves fetch only an
  index past the end; an empty world (no ray and no record below level 0); fuel 0 and RTC_MAX_FUEL; trace and shadow chunks in one
  launch; three frames queued back to back on one renderer (a cursor left over from the frame before would skip or repeat chunks);

  the container-pass decision, !(transparency == 0.0) of the hit primitive's material row: a glass plane in the kernel arguments and one in the record table, glass sphere / cube / closed cylinder, with the
  tables in LDS and in memory and with the program read from memory, glass triangles of a mesh, a CSG group with a glass child,
  transparency -0.0 (no container pass) and NaN (a container pass: !(NaN == 0.0)); fuel 1 as well, whose last level decides nothing;

  the shade record's material row and ray index, which the builds that time frames load with its point in front of the shadow rays
  (wf_shadow_rec<.., EARLY>) and the counting builds behind them: records with and without colour
  rows, the NaN-reflectance blend of a glass mirror, and the area-light reader, at level 0 and below.

Every case renders the wavefront path and the one-kernel path and requires the same bits -- pixels, primary hits, hit-tree digests -- and
compares with the oracle (parity.py) wherever the oracle answers: it has no area lights, and a NaN transparency is compared between the
paths only."""
import dataclasses
import math
import os
import re

import numpy as np

import cases
import wf_shade_queues as q
from parity import assert_parity
from raytracer_challenge_amd import scenes
from raytracer_challenge_amd.scene import Camera, Color, Element, Material, Matrix, Pattern, PointLight, ShapeArgs, Vector, World

with open(os.path.join(os.path.dirname(scenes.__file__), "csrc", "device_scene.h")) as _f:
    MAX_FUEL = int(re.search(r"^#define RTC_MAX_FUEL (\d+)$", _f.read(), re.M).group(1))  # the largest fuel the library accepts
CURSOR_FRAMES = ((8, 8), (56, 8), (64, 8), (72, 8))
SWITCHES = {"default": {}, "no_lds": {"RTC_WF_LDS": "0"}, "no_kops": {"RTC_NO_KOPS": "1"}}


def sized(cam, w, h):
    return Camera.new(w, h, cam.field_of_view, cam.transform_matrix)


def glass_and_mirror(w=48, h=32):
    """All-Plain glass, mirrors and matte surfaces under one light: trace and shadow chunks in every launch below level 0."""
    cam, world = q.all_plain_glass()
    return sized(cam, w, h), world


def empty_world(w, h):
    cam, world = q.all_plain_glass()
    return sized(cam, w, h), World(world.lights, [])


def _plain(r, g, b, **kw):
    return Material(pattern=Pattern.plain(Color.new(r, g, b)), **kw)


def _glass(ri=1.5, transparency=0.9, **kw):
    return _plain(0.1, 0.1, 0.15, diffuse=0.2, transparency=transparency, reflective=0.4, refractive_index=ri, **kw)


def _look():
    return Camera.new(48, 32, 1.0, Camera.transform(Vector.point(0.4, 1.8, -7), Vector.point(0, 0.8, 0), Vector.vector(0, 1, 0)))


def _matte_things():
    return [Element.sphere(ShapeArgs(transform=Matrix.translation(-1.6, 1, 1.5), material=_plain(0.8, 0.3, 0.2, reflective=0.2))),
            Element.cube(ShapeArgs(transform=Matrix.translation(1.7, 0.6, 2.0) * Matrix.rotation_y(0.5) * Matrix.scaling(0.6, 0.6, 0.6), material=_plain(0.2, 0.6, 0.3)))]


def _lights():
    return [PointLight(Color.white(), Vector.point(-6, 8, -8)), PointLight(Color.new(0.3, 0.3, 0.4), Vector.point(5, 6, -5))]


def glass_pane(n_matte_planes):
    """A glass plane between the camera and the scene, after `n_matte_planes` opaque ones: with 2 it travels in the kernel arguments
    (RTC_KPLANES = 6), with 6 it is the 7th plane and is read from the record table."""
    walls = [Element.plane(ShapeArgs(material=_plain(0.7, 0.7, 0.7, reflective=0.1))),
             Element.plane(ShapeArgs(transform=Matrix.translation(0, 0, 9) * Matrix.rotation_x(math.pi / 2), material=_plain(0.3, 0.4, 0.7)))]
    for k in range(n_matte_planes - 2):
        walls.append(Element.plane(ShapeArgs(transform=Matrix.translation(0, 0, 12 + 2 * k) * Matrix.rotation_x(math.pi / 2), material=_plain(0.5, 0.5, 0.2 + 0.1 * k))))
    pane = Element.plane(ShapeArgs(transform=Matrix.translation(0, 0, -2) * Matrix.rotation_x(math.pi / 2 - 0.2), material=_glass(1.3)))
    return _look(), World(_lights(), walls + [pane] + _matte_things())


def glass_solids(transparency=0.9):
    """A glass sphere, cube and closed cylinder (the cylinder inside the sphere's bounds: container lists two deep) over a matte floor."""
    els = [Element.plane(ShapeArgs(material=_plain(0.7, 0.7, 0.7, reflective=0.1))),
           Element.sphere(ShapeArgs(transform=Matrix.translation(-0.6, 1.1, 0) * Matrix.scaling(1.1, 1.1, 1.1), material=_glass(1.5, transparency))),
           Element.cube(ShapeArgs(transform=Matrix.translation(1.6, 0.7, -0.5) * Matrix.rotation_y(0.4) * Matrix.scaling(0.7, 0.7, 0.7), material=_glass(1.3, transparency))),
           Element.cylinder(ShapeArgs(transform=Matrix.translation(-0.4, 0.2, -0.3) * Matrix.scaling(0.4, 1, 0.4), material=_glass(1.4, transparency)), 0.0, 1.4, True)]
    return _look(), World(_lights(), els + _matte_things())


def glass_teapot():
    """assets/obj/teapot_low.obj in glass: the closest hits are triangles of a mesh BVH, which have no intersection record."""
    cam, world = scenes.chapter15_teapot("teapot_low.obj", 48, 32)
    els = [dataclasses.replace(e, material=_glass(1.5)) if e.tag == "obj" else e for e in world.elements]
    assert any(e.tag == "obj" for e in world.elements)
    return cam, World(world.lights, els)


def csg_with_glass():
    cam, world = cases.csg_scene()
    return sized(cam, 48, 32), world


TRANSPARENCY_SCENES = {
    "glass_plane_in_kernel_arguments": lambda: glass_pane(2),
    "glass_seventh_plane": lambda: glass_pane(6),
    "glass_solids": glass_solids,
}
PHONG_SCENES = {
    "plain_records": q.all_plain_glass,
    "records_with_colour_rows": q.plain_and_patterned,
    "nan_reflectance_glass_mirror": q.cone_apex_glass_mirror,
}


def set_switch(monkeypatch, name):
    for k in ("RTC_WF_LDS", "RTC_NO_KOPS"):
        monkeypatch.delenv(k, raising=False)
    for k, v in SWITCHES[name].items():
        monkeypatch.setenv(k, v)


def check(backend, orc, monkeypatch, cam, world, fuel, label, ask_oracle=True):
    """Both device paths bit for bit; the wavefront path against the oracle.  Returns the wavefront path's (rgb, hits, digests)."""
    out = q.both_paths(backend, world, cam, fuel, monkeypatch)
    if ask_oracle:
        monkeypatch.setenv("RTC_KERNEL", "4")
        assert_parity(backend, orc, world, cam, fuel, label=label)
    return out


def check_phong(backend, orc, monkeypatch, scene, fuel):
    """48x32; the glass mirror also at 47x31, where a pixel centre lies on the cone's apex and the record's colour is the NaN."""
    cam0, world = PHONG_SCENES[scene]()
    for w, h in ((48, 32), (47, 31)) if scene == "nan_reflectance_glass_mirror" else ((48, 32),):
        cam = sized(cam0, w, h)
        rgb, _, _ = check(backend, orc, monkeypatch, cam, world, fuel, "%s %dx%d fuel %d" % (scene, w, h, fuel))
        if w == 47:
            assert np.isnan(rgb[(h // 2) * w + w // 2]).all()


def container_rays(backend, world, cam, fuel, monkeypatch, make_out, **renderer_kw):
    """rays_container of one counted frame on each device path ("1": one kernel, "4": wavefront)."""
    from raytracer_challenge_amd.device import DeviceRenderer
    n = {}
    for path in ("1", "4"):
        monkeypatch.setenv("RTC_KERNEL", path)
        dr = DeviceRenderer(backend, backend.build_world(world), cam, 0, **renderer_kw)
        n[path] = dr.render_rows(fuel, 0, 1, cam.vsize, make_out(cam.vsize * cam.hsize * 3), count=True, sync=True)["rays_container"]
    return n


def three_frames_back_to_back(backend, world, cam, fuel, monkeypatch, make_out, **renderer_kw):
    """Three frames queued on one renderer without a sync in between, each into its own buffer: all equal to a synchronous render."""
    from raytracer_challenge_amd.device import DeviceRenderer
    monkeypatch.setenv("RTC_KERNEL", "4")
    nw = backend.build_world(world)
    want, _ = backend.render(nw, cam, fuel)
    dr = DeviceRenderer(backend, nw, cam, 0, **renderer_kw)
    outs = [make_out(cam.vsize * cam.hsize * 3) for _ in range(3)]
    for o in outs:
        dr.render_rows_async(fuel, 0, 1, cam.vsize, o)
    dr.sync()
    dr.check()
    for k, o in enumerate(outs):
        got = o.cpu().numpy().reshape(-1, 3)
        assert np.array_equal(got.view(np.uint64), want.view(np.uint64)), "frame %d of three differs from a synchronous render" % k
