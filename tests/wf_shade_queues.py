"""Cases shared by test_wf_shade_queues_cpu.py (the emulated kernels) and test_wf_shade_queues_gpu.py: what wf_shade hands to the
traversal kernel -- shade records, with or without colour rows, and the next level's rays -- at the sizes where its loop changes shape.

Cameras: 1x1 (one lane, the rest of its block idle); 7x5 (no tile padding: hsize < 8); 23x23 (576 padded work ids: one full 512-item
block iteration and a tail of 64, so a block's prefetch of the next iteration runs past the level's end); 64x36 (several iterations
of several blocks).  Fuel 0, 1, 5 and 16 (RTC_MAX_FUEL).

Every case renders the wavefront path and the one-kernel path and requires the same bits; the oracle is asked wherever it can answer:
it re-traces every secondary subtree once per light, so at fuel 16 a scene with two lights and materials that both reflect and refract
costs it up to 4^16 traces per pixel.  Those cases (nested_glass, glass_cluster at fuel 16) run on the 7x5 camera and compare the two
device paths only; every other case is also checked against the oracle."""
import dataclasses
import math

import numpy as np

import cases
from parity import assert_parity
from raytracer_challenge_amd.scene import Camera, Color, Element, Material, Matrix, Pattern, PointLight, ShapeArgs, Vector, World

CAMERAS = {"1x1": (1, 1), "7x5": (7, 5), "23x23": (23, 23), "64x36": (64, 36)}


def _look(frm, to, fov=1.0):
    return Camera.new(8, 8, fov, Camera.transform(Vector.point(*frm), Vector.point(*to), Vector.vector(0, 1, 0)))


def nothing_in_view():
    """Level 0 has no hit: the only shape is behind the camera."""
    world = World([PointLight(Color.white(), Vector.point(-5, 5, -5))], [Element.sphere(ShapeArgs(transform=Matrix.translation(0, 0, -10)))])
    return _look((0, 0, -5), (0, 0, 0)), world


def all_matte():
    """cases.all_primitives with nothing reflective: level 0 spawns no rays, the levels below run on empty queues."""
    cam, world = cases.all_primitives()
    els = [dataclasses.replace(e, args=dataclasses.replace(e.args, material=dataclasses.replace(e.args.material, reflective=0.0, transparency=0.0)))
           for e in world.elements]
    return cam, World(world.lights, els)


def cone_apex_glass_mirror():
    """The apex hit of a reflective and transparent cone has a NaN reflectance, which becomes the record's colour (odd cameras have a
    pixel centre on the apex)."""
    world, _ = cases.cone_apex_world(1, glass_mirror=True)
    return _look((0, 0, -5), (0, 0, 0), 0.5), world


def plain_and_patterned():
    """Plain and patterned materials side by side -- records with and without colour rows in one block, behind mirrors and glass too."""
    plain = lambda r, g, b, **kw: Material(pattern=Pattern.plain(Color.new(r, g, b)), **kw)
    check = Pattern.checkers(Matrix.scaling(0.5, 0.5, 0.5), Pattern.plain(Color.white()), Pattern.plain(Color.new(0.1, 0.1, 0.3)))
    stripes = Pattern.stripes(Matrix.scaling(0.2, 1, 1), Pattern.plain(Color.new(0.9, 0.3, 0.1)), Pattern.plain(Color.new(0.1, 0.7, 0.3)))
    els = [Element.plane(ShapeArgs(material=Material(pattern=check, reflective=0.3))),
           Element.plane(ShapeArgs(transform=Matrix.translation(0, 0, 6) * Matrix.rotation_x(math.pi / 2), material=plain(0.3, 0.5, 0.8, reflective=0.2))),
           Element.sphere(ShapeArgs(transform=Matrix.translation(-1.5, 1, 0), material=plain(0.8, 0.2, 0.2, reflective=0.4))),
           Element.sphere(ShapeArgs(transform=Matrix.translation(1.5, 1, 0), material=Material(pattern=stripes, specular=0.3))),
           Element.sphere(ShapeArgs(transform=Matrix.translation(0, 0.8, -1.5) * Matrix.scaling(0.8, 0.8, 0.8),
                                    material=plain(0.05, 0.05, 0.1, diffuse=0.2, transparency=0.9, reflective=0.5, refractive_index=1.5))),
           Element.cube(ShapeArgs(transform=Matrix.translation(0, 0.5, 2.5) * Matrix.scaling(0.5, 0.5, 0.5),
                                  material=Material(pattern=stripes, transparency=0.6, reflective=0.3, refractive_index=1.3)))]
    return _look((0.3, 2.5, -6), (0, 0.8, 0), 1.1), World([PointLight(Color.white(), Vector.point(-6, 8, -8))], els)


def all_plain_glass():
    """plain_and_patterned with every material Plain: the all-Plain kernels (wf_shade's pipelined build), mirrors and glass included."""
    cam, world = plain_and_patterned()
    grey = Pattern.plain(Color(0.6, 0.5, 0.4))
    els = [e if e.args.material.pattern.tag == "plain" else
           dataclasses.replace(e, args=dataclasses.replace(e.args, material=dataclasses.replace(e.args.material, pattern=grey))) for e in world.elements]
    return cam, World(world.lights, els)


SCENES = {
    "all_plain_glass": all_plain_glass,
    "nested_glass": cases.nested_glass,                # total internal reflection; reflected plus refracted children
    "glass_cluster": cases.glass_cluster,
    "nothing_in_view": nothing_in_view,
    "all_matte": all_matte,
    "cone_apex_glass_mirror": cone_apex_glass_mirror,
    "patterns_and_noise": cases.patterns_and_noise,
    "plain_and_patterned": plain_and_patterned,
}
ORACLE_TOO_DEEP = ("nested_glass", "glass_cluster")   # at fuel 16 (see the module docstring)


def case_list(scenes):
    """(scene, camera, fuel, ask the oracle): every camera at fuel 5, every other fuel at 23x23."""
    out = [(s, c, 5, True) for s in scenes for c in CAMERAS]
    for s in scenes:
        for fuel in (0, 1, 16):
            deep = fuel == 16 and s in ORACLE_TOO_DEEP
            out.append((s, "7x5" if deep else "23x23", fuel, not deep))
    return out


def sized(cam, name):
    w, h = CAMERAS[name]
    return Camera.new(w, h, cam.field_of_view, cam.transform_matrix)


def both_paths(backend, world, cam, fuel, monkeypatch):
    """rgb (as bits, so that a NaN equals the same NaN), primary hits and digests of the two device paths; asserts they are equal."""
    out = {}
    for path in ("1", "4"):
        monkeypatch.setenv("RTC_KERNEL", path)
        nw = backend.build_world(world)
        rgb, hits = backend.render(nw, cam, fuel)
        out[path] = (rgb.copy(), hits.copy(), backend.render_digest(nw, cam, fuel).copy())
    a, b = out["1"], out["4"]
    assert np.array_equal(a[0].view(np.uint64), b[0].view(np.uint64)), "rgb differs between the paths at pixels %s" % np.flatnonzero((a[0].view(np.uint64) != b[0].view(np.uint64)).any(axis=1))[:5]
    assert a[1].tobytes() == b[1].tobytes(), "primary hits differ between the paths"
    assert np.array_equal(a[2], b[2]), "digests differ between the paths"
    return b


def check_case(backend, orc, monkeypatch, scene, camera, fuel, ask_oracle):
    cam, world = SCENES[scene]()
    cam = sized(cam, camera)
    rgb, hits, _ = both_paths(backend, world, cam, fuel, monkeypatch)
    if scene == "cone_apex_glass_mirror" and cam.hsize % 2 == 1 and cam.vsize % 2 == 1:
        assert np.isnan(rgb[(cam.vsize // 2) * cam.hsize + cam.hsize // 2]).all()
    if scene == "nothing_in_view":
        assert (hits["prim"] == -1).all() and not rgb.any()
    if ask_oracle:
        monkeypatch.setenv("RTC_KERNEL", "4")
        assert_parity(backend, orc, world, cam, fuel, label="%s %s fuel %d" % (scene, camera, fuel))
