"""Cases shared by test_wf_level_classes_cpu.py (the emulated kernels) and test_wf_level_classes_gpu.py: the wavefront path's two-ended
queues (csrc/device_scene.h DWave).  A level's rays off curved primitives -- reflected ones, then refracted ones -- and its shade records
off planes are reserved from the far end of their queue down, everything else from index 0 up; whatever loops over a level walks the
far end first and cuts each part into its own 64-item chunks.  Where a ray sits in its queue is invisible to the results, so every case asks for the one-kernel path's bits.

Scenes: the smoke-size synthetic analytic scene (3 mirror planes, 64 primitives of which some are glass that also reflects) and cuts
of it that empty one end at a time -- no glass (no ray is ever refracted: the far end of a ray queue holds one class), only glass and
no planes (no record lies on a plane, no ray leaves one: the near end of every queue below level 0 is empty), planes only (both far
ends empty) -- and a small glass-and-mirror scene under the 7x5 camera, whose 35 primary rays leave each part of level 1 a single partial chunk.

Cameras: 1x1, 7x5 (35 work ids, no tile padding), 23x23 (576 padded work ids) and 64x36 (2 304).  Fuel 0, 1, 2, 5 and 16.

The oracle re-traces every secondary subtree once per light; with two lights, and glass that also reflects, fuel 16 costs it up to
4^16 traces per pixel.  The fuel-16 cases therefore run on the 7x5 camera and compare the two device paths only, as the fuel-16 glass
cases of wf_shade_queues.py do; every other case is also held to the oracle, on all of its pixels."""
import ctypes as C
import dataclasses

import numpy as np

import wf_shade_queues as q
from parity import assert_parity
from raytracer_challenge_amd import scenes
from raytracer_challenge_amd.cabi import HIT_DTYPE, RtcStatsC
from raytracer_challenge_amd.scene import Camera, Color, Element, Material, Matrix, Pattern, PointLight, ShapeArgs, Vector, World

CAMERAS = q.CAMERAS
FUELS = (0, 1, 2, 5, 16)


def _base():
    return scenes.synthetic_analytic(n_primitives=64, seed=12345, cones=False, grouped=False, hsize=64, vsize=36)


def _with_material(e, **kw):
    return dataclasses.replace(e, args=dataclasses.replace(e.args, material=dataclasses.replace(e.args.material, **kw)))


def no_glass():
    cam, world = _base()
    assert any(e.args.material.transparency > 0.0 for e in world.elements)
    return cam, World(world.lights, [_with_material(e, transparency=0.0) if e.args.material.transparency > 0.0 else e for e in world.elements])


def glass_only():
    cam, world = _base()
    body = [_with_material(e, diffuse=0.3, transparency=0.9, refractive_index=1.5, reflective=0.9) for e in world.elements[3:]]
    return cam, World(world.lights, body)


def planes_only():
    cam, world = _base()
    return cam, World(world.lights, world.elements[:3])


SCENES = {"base": _base, "no_glass": no_glass, "glass_only": glass_only, "planes_only": planes_only, "small_parts": q.all_plain_glass}


def case_list():
    """(scene, camera, fuel, ask the oracle): every camera at fuel 5, the other fuels at 23x23 (fuel 16: 7x5, the device paths only);
    small_parts is about its 7x5 camera and runs on it at every fuel."""
    out = []
    for s in SCENES:
        if s == "small_parts":
            out += [(s, "7x5", f, f != 16) for f in FUELS]
            continue
        out += [(s, c, 5, True) for c in CAMERAS]
        out += [(s, "7x5" if f == 16 else "23x23", f, f != 16) for f in FUELS if f != 5]
    return out


def scene_camera(scene, camera):
    cam, world = SCENES[scene]()
    w, h = camera if isinstance(camera, tuple) else CAMERAS[camera]
    return Camera.new(w, h, cam.field_of_view, cam.transform_matrix), world


def check_case(backend, orc, monkeypatch, scene, camera, fuel, ask_oracle):
    cam, world = scene_camera(scene, camera)
    q.both_paths(backend, world, cam, fuel, monkeypatch)
    if ask_oracle:
        monkeypatch.setenv("RTC_KERNEL", "4")
        assert_parity(backend, orc, world, cam, fuel, label="%s %s fuel %d" % (scene, camera, fuel))


RAY_COUNTERS = ("rays_primary", "rays_shadow", "rays_reflect", "rays_refract", "rays_container")


def ray_counters(backend, world, cam, fuel, path, monkeypatch, tensor):
    """The ray counters of one counting frame on device path `path`, and the frame.  tensor(n): a float64 buffer where the backend renders."""
    from raytracer_challenge_amd.device import DeviceRenderer
    monkeypatch.setenv("RTC_KERNEL", path)
    dr = DeviceRenderer(backend, backend.build_world(world), cam, 0, _cpu_standin=backend.name == "hip-emu-cpu")
    out = tensor(cam.vsize * cam.hsize * 3)
    st = dr.render_rows(fuel, 0, 1, cam.vsize, out, count=True, sync=True)
    return {k: st[k] for k in RAY_COUNTERS}, out.cpu().numpy().reshape(-1, 3).copy()


# ---- the two ends of a queue meeting ---------------------------------------------------------------------------------------------------
# Explicit rays into a closed room of six mirror planes with one sphere of glass that also reflects, one light, fuel 1.  A ray aimed at
# the sphere has two children (both at the far end of level 1's queue: the reflected one, then the refracted one), a ray aimed at the
# floor has one (at the near end), and every child hits something: the refracted ones the sphere from inside, the others a plane.  With
# n rays of which g go to the sphere, level 1 holds 2 g rays at the far end and n - g at the near end, and as many shade records (n on
# planes from index 0 up, the refracted rays' g records on the sphere from the far end down).  The queues of a launch of n work ids
# hold cap(n) items: g = cap - n makes both ends of the ray queue, and both ends of level 1's record queue, meet exactly; g + 1 makes the ray queue's ends cross by one item.  (The record
# queue cannot be made to cross on its own: a level has no more records than rays.)
def meeting_room():
    mirror = Material(pattern=Pattern.plain(Color.new(0.4, 0.5, 0.6)), reflective=0.5)
    wall = lambda t: Element.plane(ShapeArgs(transform=t, material=mirror))
    half_pi = np.pi / 2.0
    els = [wall(Matrix.id()), wall(Matrix.translation(0, 12, 0)),
           wall(Matrix.translation(0, 0, 30) * Matrix.rotation_x(half_pi)), wall(Matrix.translation(0, 0, -30) * Matrix.rotation_x(half_pi)),
           wall(Matrix.translation(30, 0, 0) * Matrix.rotation_z(half_pi)), wall(Matrix.translation(-30, 0, 0) * Matrix.rotation_z(half_pi)),
           Element.sphere(ShapeArgs(transform=Matrix.translation(0, 4, 0) * Matrix.scaling(2, 2, 2),
                                    material=Material(pattern=Pattern.plain(Color.new(0.1, 0.1, 0.2)), diffuse=0.3, transparency=0.9, refractive_index=1.5, reflective=0.5)))]
    return World([PointLight(Color.white(), Vector.point(-10, 10, -10))], els)


def meeting_rays(n, g):
    """n rays: the first g at the sphere (from z = -10, within 0.5 of its axis), the others straight down at the floor beside it."""
    k = np.arange(n, dtype=np.float64)
    rays = np.empty((n, 6))
    rays[:g] = np.stack([0.5 * np.cos(k[:g]), 4.0 + 0.5 * np.sin(k[:g]), np.full(g, -10.0), np.zeros(g), np.zeros(g), np.ones(g)], axis=1)
    m = n - g
    rays[g:] = np.stack([5.0 + 20.0 * (k[g:] - g) / max(1, m), np.full(m, 6.0), 10.0 * np.sin(k[g:]), np.zeros(m), -np.ones(m), np.zeros(m)], axis=1)
    return rays


def trace_rays(backend, world, rays, fuel, path, monkeypatch):
    """(rgb, hits, stats, the scene's error state afterwards) of include/rtc.h rtc_trace_rays on device path `path`, a fresh scene."""
    lib = backend.lib
    vp = C.c_void_p
    monkeypatch.setenv("RTC_KERNEL", path)
    nw = backend.build_world(world)
    scene = lib.rtw_world_scene(nw.handle, 0)
    assert scene, backend._err()
    rays = np.ascontiguousarray(rays, dtype=np.float64)
    n = len(rays)
    rgb, hits, st = np.empty((n, 3)), np.empty(n, dtype=HIT_DTYPE), RtcStatsC()
    assert lib.rtc_trace_rays(scene, rays.ctypes.data, n, fuel, rgb.ctypes.data, hits.ctypes.data, C.byref(st)) == 0, lib.rtc_last_error()
    check = lib.rtc_scene_check(scene)
    out = (rgb.copy(), hits.copy(), st.as_dict(), check)
    nw.close()
    return out


def check_ends_meet(backend, monkeypatch, n, cap, over):
    """n rays of which cap - n (+ 1 if over) go to the sphere, both paths: the same bits, the counters of the construction above, no error
    left behind.  Returns the wavefront path's result."""
    g = cap - n + (1 if over else 0)
    assert 0 < g < n
    world, rays = meeting_room(), meeting_rays(n, g)
    one = trace_rays(backend, world, rays, 1, "1", monkeypatch)
    wf = trace_rays(backend, world, rays, 1, "4", monkeypatch)
    assert np.array_equal(one[0].view(np.uint64), wf[0].view(np.uint64)), "pixels differ between the paths"
    assert one[1].tobytes() == wf[1].tobytes(), "hit records differ between the paths"
    assert (wf[1]["prim"][:g] == 6).all() and (wf[1]["prim"][g:] == 0).all()
    for st in (one[2], wf[2]):
        assert (st["rays_primary"], st["rays_reflect"], st["rays_refract"]) == (n, n, g), st   # level 1: n - g at the near end, 2 g at the far end
    assert wf[2]["rays_shadow"] == n + n + g, wf[2]   # one light: every ray of both levels left a shade record (level 1: n on planes, g not)
    assert one[3] == 0 and wf[3] == 0, "an error state was left behind"
    return wf
