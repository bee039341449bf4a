"""The sampled camera (include/rtc.h rtc_sampling) on an MI355X, both device paths.  The oracle restates the reference, which has one
ray per pixel, so the semantics are pinned through identities: an unjittered 2x2 / 4x4 grid is the pixel set of a camera of 2x / 4x the
resolution; the device's rays are the host evaluation's (test_sampled_camera_cpu.py compares that with a restatement); a sampled pixel
is the k-ordered mean of rtc_trace_rays over exactly those rays; side 1 is rtc_render; chunks, bands, replicas and the Python layers
change no bit; a wall in the focal plane is sharp through any lens."""
import ctypes as C
import math

import numpy as np
import pytest

import cases
import foreign_flattener as ff
from raytracer_challenge_amd import scenes
from raytracer_challenge_amd.backend import SamplingC
from raytracer_challenge_amd.device import DeviceRenderer, RtcStatsC
from raytracer_challenge_amd.image import Image
from raytracer_challenge_amd.parallel import rows_of
from raytracer_challenge_amd.scene import Camera, Color, Element, Material, Matrix, Pattern, PointLight, Sampling, ShapeArgs, Vector, World
from test_area_lights_gpu import mirror_world, penumbra_world
from test_sampled_camera_cpu import block_mean, samples_mean

pytestmark = pytest.mark.gpu
PATHS = ["1", "4"]
vp = C.c_void_p


def resized(cam, w, h):
    return Camera.new(w, h, cam.field_of_view, cam.transform_matrix)


def sampled(lib, scene, cam, sp, fuel, idx=None, stats=None):
    """rtc_render_sampled through C: the whole frame or the listed pixels."""
    rc, spc = ff.make_camera(cam), SamplingC.of(sp)
    idx_a = None if idx is None else np.ascontiguousarray(idx, dtype=np.uint64)
    n = cam.hsize * cam.vsize if idx is None else idx_a.size
    rgb = np.full((n, 3), np.nan)
    code = lib.rtc_render_sampled(scene, C.byref(rc), C.byref(spc), fuel, None if idx is None else idx_a.ctypes.data, 0, n, rgb.ctypes.data,
                                  None if stats is None else C.byref(stats))
    assert code == 0, lib.rtc_last_error()
    return rgb


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


# ---- 1. against the oracle: an unjittered power-of-two grid is the pixel set of a finer camera -------------------------------------
_fine = {}


def fine_frame(orc, name):
    """The oracle's 96x64 render of the scene at fuel 5, once."""
    if name not in _fine:
        cam, world = getattr(scenes, name)(96, 64)
        _fine[name] = orc.render(orc.build_world(world), cam, 5)[0]
    return _fine[name]


@pytest.mark.parametrize("name", ["cover", "chapter11_title"])
@pytest.mark.parametrize("path", PATHS)
def test_grid_is_the_finer_cameras_pixels(hip, orc, path, name, monkeypatch):
    monkeypatch.setenv("RTC_KERNEL", path)
    cam96, world = getattr(scenes, name)(96, 64)
    nw = hip.build_world(world)
    own = hip.render(nw, cam96, 5, want_hits=False)[0]
    ref = fine_frame(orc, name)
    for side in (4, 2):   # the sampled 24x16 (48x32) frame: 4x4 (2x2) blocks of the 96x64 frame
        w, h = 96 // side, 64 // side
        got = hip.render_sampled(nw, resized(cam96, w, h), Sampling(side=side), 5)
        assert np.array_equal(bits(got), bits(block_mean(own, w, h, side))), (name, side)
        err = float(np.abs(got - block_mean(ref, w, h, side)).max())
        print("%s path %s side %d: max |dRGB| vs the oracle's block mean = %.3e" % (name, path, side, err))
        assert err <= 1e-5, (name, side, err)


# ---- 2. the device's rays are the host evaluation's --------------------------------------------------------------------------------
@pytest.mark.parametrize("path", PATHS)
def test_device_rays_are_the_host_rays(hip, path, monkeypatch):
    monkeypatch.setenv("RTC_KERNEL", path)
    cam, world = scenes.chapter11_glass_air_bubble(37, 19)
    nw = hip.build_world(world)
    idx = np.array([702, 0, 36, 37, 350, 350, 1], dtype=np.uint64)
    for side in (1, 3, 16):
        for jit in (False, True):
            sp = Sampling(side=side, jitter=jit, seed=42 + side)
            pixels = idx if side == 16 else None   # side 16: the pixel list (a list launch); else the whole frame (a row launch)
            dev, host = hip.camera_rays(cam, sp, pixel_indices=pixels, nw=nw), hip.camera_rays(cam, sp, pixel_indices=pixels)
            assert dev.shape == ((7 if side == 16 else 703), side * side, 6)
            assert np.array_equal(bits(dev), bits(host)), (side, jit)
        assert np.array_equal(bits(hip.camera_rays(cam, Sampling(side=side), pixel_indices=idx, nw=nw)), bits(hip.camera_rays(cam, Sampling(side=side), pixel_indices=idx)))
    for side, jit, R, F in ((1, False, 0.05, 1.0), (3, True, 0.2, 4.5), (16, True, 1.5, 0.3)):
        sp = Sampling(side=side, jitter=jit, seed=9, lens_radius=R, focal_distance=F)
        pixels = idx if side == 16 else None
        err = float(np.abs(hip.camera_rays(cam, sp, pixel_indices=pixels, nw=nw) - hip.camera_rays(cam, sp, pixel_indices=pixels)).max())
        assert err <= 1e-12, (side, R, F, err)   # cos / sin: the device's library against the host's


# ---- 3. a sampled pixel is the mean of World::color_at over exactly those rays -----------------------------------------------------
def scene_of(name):
    if name == "glass_and_mirror":
        return Camera.new(8, 8, 1.0, Camera.transform(Vector.point(0.0, 3.0, -7.0), Vector.point(0.0, 0.7, 0.0), Vector.vector(0.0, 1.0, 0.0))), mirror_world()
    if name == "area_light_jittered":
        return Camera.new(8, 8, 1.0, Camera.transform(Vector.point(0.0, 3.0, -7.0), Vector.point(0.0, 0.7, 0.0), Vector.vector(0.0, 1.0, 0.0))), penumbra_world(jit=True)
    if name == "texture_showcase":
        return scenes.texture_showcase(8, 8)
    return cases.SMALL_CASES[name]()   # csg_scene, teapot_low (a mesh)


SHAPES = [  # (frame, sampling, pixel list or None)
    ((37, 19), Sampling(side=2, seed=3), [0, 351, 702]),                                             # 12 rays: a partial wave
    ((37, 19), Sampling(side=16, jitter=True, seed=4), [36, 37, 38, 400, 702]),
    ((9, 9), Sampling(side=3, jitter=True, seed=5), None),
    ((37, 19), Sampling(side=2, jitter=True, seed=6, lens_radius=0.2, focal_distance=6.0), None),
]


@pytest.mark.parametrize("name", ["glass_and_mirror", "csg_scene", "teapot_low", "area_light_jittered", "texture_showcase"])
@pytest.mark.parametrize("path", PATHS)
def test_pixels_are_the_mean_of_their_rays(hip, path, name, monkeypatch):
    monkeypatch.setenv("RTC_KERNEL", path)
    cam0, world = scene_of(name)
    nw = hip.build_world(world)
    for (w, h), sp, pixels in SHAPES:
        cam = resized(cam0, w, h)
        idx = None if pixels is None else np.array(pixels, dtype=np.uint64)
        rays = hip.camera_rays(cam, sp, pixel_indices=idx, nw=nw)
        colours, _ = hip.color_at(nw, rays.reshape(-1, 6), 5)
        got = hip.render_sampled(nw, cam, sp, 5, pixel_indices=idx)
        want = samples_mean(colours.reshape(rays.shape[0], sp.samples, 3))
        assert np.array_equal(bits(got), bits(want)), (name, (w, h), sp)
        assert np.isfinite(got).all() and (pixels is not None or got.max() > 0.0), (name, (w, h))


# ---- 4. identity with today ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("path", PATHS)
def test_one_centre_sample_is_rtc_render_and_counters(hip, path, monkeypatch):
    monkeypatch.setenv("RTC_KERNEL", path)
    lib = hip.lib
    cam, world = scenes.chapter11_glass_air_bubble(40, 24)
    nw = hip.build_world(world)
    scene = lib.rtw_world_scene(nw.handle, 0)
    plain = hip.render(nw, cam, 5, want_hits=False)[0]
    assert np.array_equal(bits(sampled(lib, scene, cam, Sampling(), 5)), bits(plain))
    idx = np.array([959, 3, 500], dtype=np.uint64)
    assert np.array_equal(bits(sampled(lib, scene, cam, Sampling(seed=77), 5, idx=idx)), bits(plain[idx.astype(np.int64)]))
    st = RtcStatsC()
    a = sampled(lib, scene, cam, Sampling(side=3), 5, stats=st)
    assert st.pixels == 960 and st.rays_primary == 960 * 9 and st.kernel_ms > 0.0
    assert st.n_launches == (2 * 5 + 4 if path == "4" else 1) + 2     # one chunk: the trace launches, the generator and the resolve
    assert np.array_equal(bits(a), bits(sampled(lib, scene, cam, Sampling(side=3), 5)))   # the counting kernels give the same pixels
    st2 = RtcStatsC()
    sampled(lib, scene, cam, Sampling(side=3), 5, idx=idx, stats=st2)
    assert st2.pixels == 3 and st2.rays_primary == 27


# ---- 5. chunks and partitions change no bit ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("path", PATHS)
def test_chunks_change_no_bit(hip, path, monkeypatch):
    monkeypatch.setenv("RTC_KERNEL", path)
    lib = hip.lib
    cam, world = scenes.chapter11_glass_air_bubble(37, 19)
    nw = hip.build_world(world)
    scene = lib.rtw_world_scene(nw.handle, 0)
    sp = Sampling(side=3, jitter=True, seed=11)
    idx = np.arange(702, 2, -3, dtype=np.uint64)   # 234 pixels
    whole, listed = sampled(lib, scene, cam, sp, 5), sampled(lib, scene, cam, sp, 5, idx=idx)
    assert np.array_equal(bits(listed), bits(whole[idx.astype(np.int64)]))
    monkeypatch.setenv("RTC_SAMPLED_MAX_RAYS", "1000")   # 3 rows of 333 rays per chunk: 7 chunks; 111 listed pixels per chunk: 3 chunks
    st = RtcStatsC()
    assert np.array_equal(bits(sampled(lib, scene, cam, sp, 5, stats=st)), bits(whole))
    assert st.pixels == 703 and st.rays_primary == 703 * 9
    assert st.n_launches == 7 * ((2 * 5 + 4 if path == "4" else 1) + 2)
    assert np.array_equal(bits(sampled(lib, scene, cam, sp, 5)), bits(whole))
    assert np.array_equal(bits(sampled(lib, scene, cam, sp, 5, idx=idx)), bits(listed))
    monkeypatch.setenv("RTC_SAMPLED_MAX_RAYS", "1")      # never fewer than one row / one pixel
    assert np.array_equal(bits(sampled(lib, scene, cam, sp, 5)), bits(whole))
    assert np.array_equal(bits(sampled(lib, scene, cam, sp, 5, idx=idx[:5])), bits(listed[:5]))


@pytest.mark.parametrize("path", PATHS)
def test_partitions_and_layers_change_no_bit(hip, path, monkeypatch):
    import torch
    monkeypatch.setenv("RTC_KERNEL", path)
    lib = hip.lib
    world = mirror_world()
    cam = Camera.new(40, 24, 1.0, Camera.transform(Vector.point(0.0, 3.0, -7.0), Vector.point(0.0, 0.7, 0.0), Vector.vector(0.0, 1.0, 0.0)))
    sp = Sampling(side=2, jitter=True, seed=21, lens_radius=0.1, focal_distance=7.0)
    nw = hip.build_world(world)
    scene = lib.rtw_world_scene(nw.handle, 0)
    whole = sampled(lib, scene, cam, sp, 5)
    rc, spc = ff.make_camera(cam), SamplingC.of(sp)
    # two replicas on one device
    flat = ff.flatten(world)
    desc = flat.desc()
    m, devs = vp(), (C.c_int * 2)(0, 0)
    assert lib.rtc_multi_create(C.byref(desc), devs, 2, C.byref(m)) == 0, lib.rtc_last_error()
    mrgb, st = np.full((960, 3), np.nan), RtcStatsC()
    assert lib.rtc_render_multi_sampled(m, C.byref(rc), C.byref(spc), 5, mrgb.ctypes.data, None) == 0, lib.rtc_last_error()
    assert np.array_equal(bits(mrgb), bits(whole))
    mrgb[:] = np.nan
    assert lib.rtc_render_multi_sampled(m, C.byref(rc), C.byref(spc), 5, mrgb.ctypes.data, C.byref(st)) == 0, lib.rtc_last_error()
    lib.rtc_multi_destroy(m)
    assert np.array_equal(bits(mrgb), bits(whole)) and st.pixels == 960 and st.rays_primary == 960 * 4
    # bands of 8 rows dealt to two parts, left on the device
    dr = DeviceRenderer(hip, nw, cam)
    frame = np.full((24, 40, 3), np.nan)
    for part in (0, 1):
        rows = rows_of(part, 2, 24, 8)
        t = torch.full((len(rows) * 40 * 3,), float("nan"), dtype=torch.float64, device="cuda:0")
        torch.cuda.synchronize()   # the fill runs on torch's stream, the render on the scene's
        if part == 0:
            d = dr.render_rows(5, part, 2, len(rows), t, band_rows=8, sampling=sp)
            assert d["pixels"] == len(rows) * 40
        else:
            dr.render_rows_async(5, part, 2, len(rows), t, band_rows=8, sampling=sp)
            dr.check()
        frame[rows] = t.cpu().numpy().reshape(len(rows), 40, 3)
    assert np.array_equal(bits(frame.reshape(-1, 3)), bits(whole))
    # the Python layers
    assert np.array_equal(bits(hip.render_sampled(nw, cam, sp, 5)), bits(whole))
    img = Image.par_render(cam, world, sampling=sp)
    assert (img.hsize, img.vsize) == (40, 24) and np.array_equal(bits(np.asarray(img.pixels).reshape(-1, 3)), bits(whole))
    # quantised on the device
    rgb8, q = np.zeros(whole.size, dtype=np.uint8), np.zeros(whole.size, dtype=np.uint8)
    assert lib.rtc_render_sampled_rgb8(scene, C.byref(rc), C.byref(spc), 5, rgb8.ctypes.data, None) == 0, lib.rtc_last_error()
    assert lib.rtc_quantize(scene, np.ascontiguousarray(whole).ctypes.data, whole.size, q.ctypes.data) == 0, lib.rtc_last_error()
    assert np.array_equal(rgb8, q) and rgb8.max() > 0


# ---- 6. focus ------------------------------------------------------------------------------------------------------------------------
def wall_world(depth):
    """A wall facing the camera (at the origin, looking down -z) at camera-space depth `depth`, lit by its ambient term alone, with a
    gradient along x that has no seam inside the view."""
    pat = Pattern.gradient(Matrix.translation(-5.0, 0.0, 0.0) * Matrix.scaling(10.0, 10.0, 10.0), Pattern.plain(Color(1.0, 0.2, 0.0)), Pattern.plain(Color(0.0, 0.4, 1.0)))
    wall = Element.plane(ShapeArgs(transform=Matrix.translation(0.0, 0.0, -depth) * Matrix.rotation_x(math.pi / 2.0),
                                   material=Material(pattern=pat, ambient=1.0, diffuse=0.0, specular=0.0)))
    return World([PointLight(Color(1.0, 1.0, 1.0), Vector.point(0.0, 0.0, 0.0))], [wall])


@pytest.mark.parametrize("path", PATHS)
def test_the_focal_plane_is_sharp(hip, path, monkeypatch):
    monkeypatch.setenv("RTC_KERNEL", path)
    F = 4.0
    cam = Camera.new(32, 20, 1.0, Matrix.id())
    lens, pinhole = Sampling(side=2, jitter=True, seed=8, lens_radius=0.3, focal_distance=F), Sampling(side=2, jitter=True, seed=8)
    nw = hip.build_world(wall_world(F))
    a, b = hip.render_sampled(nw, cam, lens, 5), hip.render_sampled(nw, cam, pinhole, 5)
    assert b.min() >= 0.0 and b.max() > 0.5 and np.ptp(b[:, 0]) > 0.2    # the gradient is there
    assert float(np.abs(a - b).max()) <= 1e-9                            # every lens ray of a sample meets the wall at one point
    nw2 = hip.build_world(wall_world(2.0 * F))
    a2, b2 = hip.render_sampled(nw2, cam, lens, 5), hip.render_sampled(nw2, cam, pinhole, 5)
    assert float(np.abs(a2 - b2).max()) > 1e-3                           # out of focus: blurred


# ---- 7. path choice -----------------------------------------------------------------------------------------------------------------
def test_sampled_row_launches_choose_their_path(hip, monkeypatch):
    monkeypatch.delenv("RTC_KERNEL", raising=False)
    lib = hip.lib
    cam, world = scenes.chapter11_glass_air_bubble(64, 32)
    nw = hip.build_world(world)
    scene = lib.rtw_world_scene(nw.handle, 0)
    sp = Sampling(side=2)
    frames = [sampled(lib, scene, cam, sp, 5) for _ in range(4)]
    ch, t1, t4 = C.c_int32(0), C.c_double(-1.0), C.c_double(-1.0)
    lib.rtc_scene_path_info(scene, C.byref(ch), C.byref(t1), C.byref(t4))
    assert ch.value in (1, 4) and t1.value > 0.0 and t4.value > 0.0, (ch.value, t1.value, t4.value)
    assert np.array_equal(bits(sampled(lib, scene, cam, sp, 5)), bits(frames[0]))
    assert all(np.array_equal(bits(f), bits(frames[0])) for f in frames)
    # a pixel list stays on the one-kernel path, whatever was measured
    st = RtcStatsC()
    sampled(lib, scene, cam, sp, 5, idx=np.array([5, 6], dtype=np.uint64), stats=st)
    assert st.n_launches == 1 + 2
