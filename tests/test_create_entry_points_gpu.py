"""The creation matrix on an MI355X: a scene created through any of the twelve rtc_*_create* entry points with its extras empty IS
rtc_scene_create's -- the same frame bit for bit on both device paths, and for the six scene entry points the same kernel builds
(rtc_scene_kernel_info) and the same bytes on the device (a multi handle exposes neither).  rtc_*_create_ex has no descriptor lights
by contract, so it gets the same two lights as RTC_LIGHT_POINT entries of its list.  And one open cone (cos_inner = cos_outer = -1:
the factor is 1 everywhere) on light 0, with the lights once in desc->lights and once in ext->lights, is the cone-less frame."""
import ctypes as C

import numpy as np
import pytest

import build_matrix as bm
import create_cases as cc
import foreign_flattener as ff
from raytracer_challenge_amd.scene import Camera, Vector

pytestmark = pytest.mark.gpu
vp = C.c_void_p
FUEL = 2


class Created:
    """What one creation call gives: the frame's bits and, for a scene, its kernel builds on the pinned path and its device bytes."""

    def __init__(self, lib, entry, path, cam, desc, **kw):
        handle, rc = vp(), ff.make_camera(cam)
        assert cc.create(lib, entry, desc, handle, **kw) == 0, (entry, lib.rtc_last_error())
        rgb = np.full((cam.hsize * cam.vsize, 3), np.nan)
        if entry.startswith("rtc_multi"):
            assert lib.rtc_render_multi(handle, C.byref(rc), FUEL, rgb.ctypes.data, None) == 0, (entry, lib.rtc_last_error())
            self.info = self.device_bytes = None
            lib.rtc_multi_destroy(handle)
        else:
            assert lib.rtc_render(handle, C.byref(rc), FUEL, None, 0, len(rgb), rgb.ctypes.data, None, None) == 0, (entry, lib.rtc_last_error())
            k = bm.KernelInfo()
            assert lib.rtc_scene_kernel_info(handle, int(path), 0, C.byref(k)) == 0, lib.rtc_last_error()
            self.info, self.device_bytes = bytes(k), lib.rtc_scene_device_bytes(handle)
            lib.rtc_scene_destroy(handle)
        self.bits = rgb.view(np.uint64)


def fixtures():
    """The camera, the descriptor, the descriptor without its lights and those lights as an rtc_light_ex list (kept alive by the caller)."""
    cam = Camera.new(32, 24, 0.9, Camera.transform(Vector.point(0, 1.5, -5), Vector.point(0, 0.5, 0), Vector.vector(0, 1, 0)))
    flat = ff.flatten(cc.small_world())
    desc = flat.desc()
    unlit = ff.RtcSceneDesc.from_buffer_copy(desc)
    unlit.n_lights, unlit.lights = 0, C.POINTER(ff.RtcLight)()
    lights = (cc.RtcLightEx * desc.n_lights)()
    for i in range(desc.n_lights):
        lights[i].kind = 0  # RTC_LIGHT_POINT
        lights[i].intensity, lights[i].corner = desc.lights[i].intensity, desc.lights[i].origin
    return cam, flat, desc, unlit, lights


@pytest.mark.parametrize("path", ["1", "4"])
def test_empty_extras_are_rtc_scene_create(hip, path, monkeypatch):
    monkeypatch.setenv("RTC_KERNEL", path)
    lib = hip.lib
    cam, flat, desc, unlit, lights = fixtures()
    want = Created(lib, "rtc_scene_create", path, cam, desc)
    assert np.isfinite(want.bits.view(np.float64)).all() and want.bits.view(np.float64).max() > 0.0 and want.device_bytes > 0
    n = 0
    for entry in cc.ENTRIES:
        if entry.endswith("_ex"):
            variants = [dict(desc=unlit, lights=lights, n_lights=len(lights))]
        elif "_ext" in entry:
            variants = [dict(desc=desc, ext=None), dict(desc=desc, ext=cc.RtcSceneExt())]   # NULL, and zeroed
        else:
            variants = [dict(desc=desc)]
        for kw in variants:
            got = Created(lib, entry, path, cam, kw.pop("desc"), **kw)
            assert np.array_equal(got.bits, want.bits), (entry, sorted(kw))
            if not entry.startswith("rtc_multi"):
                assert got.info == want.info and got.device_bytes == want.device_bytes, (entry, sorted(kw), got.device_bytes, want.device_bytes)
            n += 1
    assert n == 2 * (1 + 1 + 4 * 2)


@pytest.mark.parametrize("path", ["1", "4"])
def test_open_cone_on_either_light_list_is_no_cone(hip, path, monkeypatch):
    monkeypatch.setenv("RTC_KERNEL", path)
    lib = hip.lib
    cam, flat, desc, unlit, lights = fixtures()
    want = Created(lib, "rtc_scene_create", path, cam, desc)
    cones = (cc.RtcLightCone * 1)(cc.RtcLightCone(0, 0, (C.c_double * 3)(0.0, -1.0, 0.0), -1.0, -1.0))
    ext = cc.RtcSceneExt()
    ext.n_lights, ext.lights = len(lights), lights
    for entry in [e for e in cc.ENTRIES if cc.carries(e, "cone")]:
        on_desc = Created(lib, entry, path, cam, desc, cones=cones, n_cones=1)
        on_ext = Created(lib, entry, path, cam, unlit, ext=ext, cones=cones, n_cones=1)
        assert np.array_equal(on_desc.bits, want.bits), entry
        assert np.array_equal(on_ext.bits, want.bits), entry
