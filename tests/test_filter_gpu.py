"""Pixel reconstruction filters (include/rtc.h rtc_filter) on an MI355X, both device paths.  The gather kernel is held against the host
evaluation of the same function (test_filter_cpu.py compares that with a restatement) on sample colours that were never traced -- both
of its branches, awkward frames --; a rendered frame is that function over rtc_trace_rays of exactly rtc_camera_rays' rays; an unjittered
4x4 grid ties it to the oracle's 96x64 frame; the box of half a pixel is rtc_render_sampled; chunks, row ranges, the quantiser and the
Python layers change no bit."""
import ctypes as C

import numpy as np
import pytest

import foreign_flattener as ff
from raytracer_challenge_amd import scenes
from raytracer_challenge_amd.backend import FilterC, SamplingC
from raytracer_challenge_amd.device import RtcStatsC
from raytracer_challenge_amd.image import Image
from raytracer_challenge_amd.scene import Filter, Sampling
from test_filter_cpu import bits, filters, random_samples, same_bits, window
from test_sampled_camera_gpu import fine_frame, resized

pytestmark = pytest.mark.gpu
PATHS = ["1", "4"]
vp = C.c_void_p


def filtered(lib, scene, cam, sp, flt, fuel, row_first=0, n_rows=None, stats=None):
    """rtc_render_filtered through C: the whole frame or a row range."""
    rc, spc, flc = ff.make_camera(cam), SamplingC.of(sp), FilterC.of(flt)
    n_rows = cam.vsize - row_first if n_rows is None else n_rows
    rgb = np.full((n_rows * cam.hsize, 3), np.nan)
    code = lib.rtc_render_filtered(scene, C.byref(rc), C.byref(spc), C.byref(flc), fuel, row_first, n_rows, rgb.ctypes.data, None if stats is None else C.byref(stats))
    assert code == 0, lib.rtc_last_error()
    return rgb


def traced_samples(hip, nw, cam, sp, fuel=5):
    """rtc_trace_rays over exactly the rays the device's generator makes: [pixels, N, 3]."""
    rays = hip.camera_rays(cam, sp, nw=nw)
    colours, _ = hip.color_at(nw, rays.reshape(-1, 6), fuel)
    return colours.reshape(cam.hsize * cam.vsize, sp.samples, 3)


MITCHELL_CASE = ("chapter11_glass_air_bubble", (37, 19), Sampling(side=3, jitter=True, seed=12, lens_radius=0.1, focal_distance=5.0), Filter.mitchell(2.0))


# ---- 1. the gather kernel against the host function ----------------------------------------------------------------------------------
@pytest.mark.parametrize("side", [1, 3, 4, 16])
def test_device_filter_is_the_host_function(hip, side, monkeypatch):
    """Side 16 is 256 samples per pixel, which no tile's patch fits into LDS: the memory branch.  Sides 1, 3 and 4 take the LDS branch
    for every radius above 0.5 and, with RTC_FILTER_LDS=0, the memory branch as well: the same bits."""
    monkeypatch.delenv("RTC_FILTER_LDS", raising=False)
    nw = hip.build_world(scenes.chapter11_glass_air_bubble(8, 8)[1])
    worst = 0.0
    for hsize, vsize in ((1, 1), (1, 7), (7, 1), (9, 5), (67, 13)):   # 67x13: no multiple of a tile or a wave, several blocks
        for jit in (False, True):
            sp = Sampling(side=side, jitter=jit, seed=0xBEEF + side)
            samples = random_samples(hsize, vsize, sp.samples, 100 * hsize + vsize + side, wild=True)
            for radius in (0.5, 1.5, 2.0, 3.0):
                if not jit and radius != 2.0:
                    continue   # the grid at the one radius that puts samples at a == r; the hashed positions at every radius
                for flt in filters(radius):
                    want = hip.filter_frame(samples, hsize, vsize, sp, flt)
                    got = hip.filter_frame(samples, hsize, vsize, sp, flt, nw=nw)
                    if side != 16 and radius > 0.5:
                        monkeypatch.setenv("RTC_FILTER_LDS", "0")
                        assert same_bits(hip.filter_frame(samples, hsize, vsize, sp, flt, nw=nw), got), ((hsize, vsize), side, jit, flt)
                        monkeypatch.delenv("RTC_FILTER_LDS")
                    if flt.kind == "gaussian":   # exp: the device's library against the host's
                        assert np.array_equal(np.isfinite(got), np.isfinite(want)), ((hsize, vsize), side, jit, flt)
                        ok = np.isfinite(want)
                        err = float(np.abs(got[ok] - want[ok]).max()) if ok.any() else 0.0
                        worst = max(worst, err)
                        assert err <= 1e-12, ((hsize, vsize), side, jit, flt, err)
                    else:
                        assert same_bits(got, want), ((hsize, vsize), side, jit, flt)
    print("side %d: max |device - host| over the Gaussian cases = %.3e" % (side, worst))


# ---- 2. a rendered frame is the filter over rtc_trace_rays of rtc_camera_rays' rays ------------------------------------------------
RENDER_CASES = [
    ("cover", (24, 16), Sampling(side=2, jitter=True, seed=7), Filter.tent(1.5)),
    MITCHELL_CASE,
    ("texture_showcase", (19, 9), Sampling(side=2, jitter=True, seed=9), Filter.gaussian(1.5, 2.0)),
]


@pytest.mark.parametrize("case", RENDER_CASES, ids=[c[0] for c in RENDER_CASES])
@pytest.mark.parametrize("path", PATHS)
def test_rendered_frames_are_the_filtered_traces(hip, path, case, monkeypatch):
    monkeypatch.setenv("RTC_KERNEL", path)
    name, (w, h), sp, flt = case
    cam, world = getattr(scenes, name)(w, h)
    nw = hip.build_world(world)
    got = hip.render_filtered(nw, cam, sp, flt, 5)
    want = hip.filter_frame(traced_samples(hip, nw, cam, sp), w, h, sp, flt)
    assert got.shape == (w * h, 3) and np.isfinite(got).all() and got.max() > 0.0
    if flt.kind == "gaussian":
        err = float(np.abs(got - want).max())
        print("%s path %s: max |rendered - host filter of the traces| = %.3e" % (name, path, err))
        assert err <= 1e-12, (name, err)
    else:
        assert np.array_equal(bits(got), bits(want)), name
    # and the filter did something: it is not the box mean
    assert not np.array_equal(bits(got), bits(hip.render_sampled(nw, cam, sp, 5)))


# ---- 3. the oracle link ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("path", PATHS)
def test_filtered_grid_against_the_oracles_finer_frame(hip, orc, path, monkeypatch):
    """An unjittered 4x4 grid of the 24x16 camera is the pixel set of the 96x64 camera (test_sampled_camera_gpu.py): the oracle's frame,
    rearranged into sample order and filtered by the host function, is the reference.  Tent and Gaussian weights are non-negative: a
    pixel is a convex combination of its samples and cannot amplify the 1e-5 of the colours."""
    monkeypatch.setenv("RTC_KERNEL", path)
    cam96, world = scenes.cover(96, 64)
    nw = hip.build_world(world)
    sp = Sampling(side=4)
    ref = fine_frame(orc, "cover").reshape(16, 4, 24, 4, 3).transpose(0, 2, 1, 3, 4).reshape(24 * 16, 16, 3)   # [y, x, sy, sx]: k = sy * 4 + sx
    for flt in (Filter.tent(1.5), Filter.gaussian(1.5, 2.0)):
        got = hip.render_filtered(nw, resized(cam96, 24, 16), sp, flt, 5)
        err = float(np.abs(got - hip.filter_frame(ref, 24, 16, sp, flt)).max())
        print("cover path %s %s: max |dRGB| vs the filtered oracle frame = %.3e" % (path, flt.kind, err))
        assert err <= 1e-5, (flt, err)


# ---- 4. the box of half a pixel is the sampled camera ----------------------------------------------------------------------------------
@pytest.mark.parametrize("path", PATHS)
def test_box_of_half_a_pixel_is_rtc_render_sampled(hip, path, monkeypatch):
    monkeypatch.setenv("RTC_KERNEL", path)
    cam, world = scenes.chapter11_glass_air_bubble(37, 19)
    nw = hip.build_world(world)
    for jit in (False, True):
        sp = Sampling(side=3, jitter=jit, seed=13)
        assert np.array_equal(bits(hip.render_filtered(nw, cam, sp, Filter.box(0.5), 5)), bits(hip.render_sampled(nw, cam, sp, 5))), jit


# ---- 5. partitions change no bit -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("path", PATHS)
def test_partitions_change_no_bit(hip, path, monkeypatch, capfd):
    monkeypatch.setenv("RTC_KERNEL", path)
    monkeypatch.delenv("RTC_SAMPLED_MAX_RAYS", raising=False)
    lib = hip.lib
    name, (w, h), sp, flt = MITCHELL_CASE
    cam, world = getattr(scenes, name)(w, h)
    nw = hip.build_world(world)
    scene = lib.rtw_world_scene(nw.handle, 0)
    whole = filtered(lib, scene, cam, sp, flt, 5)
    # chunks
    monkeypatch.setenv("RTC_SAMPLED_MAX_RAYS", "1000")   # 333 rays per row: fewer than the halo's 4 rows, so one output row per chunk
    assert np.array_equal(bits(filtered(lib, scene, cam, sp, flt, 5)), bits(whole))
    monkeypatch.setenv("RTC_SAMPLED_MAX_RAYS", "3000")   # 9 traced rows: 5 output rows per chunk, 4 chunks
    st = RtcStatsC()
    assert np.array_equal(bits(filtered(lib, scene, cam, sp, flt, 5, stats=st)), bits(whole))
    assert st.pixels == w * h and st.n_launches == 4 * ((2 * 5 + 4 if path == "4" else 1) + 2)
    monkeypatch.setenv("RTC_SAMPLED_MAX_RAYS", "1")
    assert np.array_equal(bits(filtered(lib, scene, cam, sp, flt, 5)), bits(whole))
    monkeypatch.delenv("RTC_SAMPLED_MAX_RAYS")
    # row ranges
    parts = [filtered(lib, scene, cam, sp, flt, 5, a, n) for a, n in ((0, 5), (5, 1), (6, 13))]
    assert np.array_equal(bits(np.concatenate(parts)), bits(whole))
    rc, spc, flc = ff.make_camera(cam), SamplingC.of(sp), FilterC.of(flt)
    out = np.zeros((w, 3))
    for a, n in ((19, 1), (0, 0), (18, 2), (5, 0)):   # outside the image or empty
        assert lib.rtc_render_filtered(scene, C.byref(rc), C.byref(spc), C.byref(flc), 5, a, n, out.ctypes.data, None) == 1, (a, n)
    # quantised on the device
    rgb8, q = np.zeros(whole.size, dtype=np.uint8), np.zeros(whole.size, dtype=np.uint8)
    assert lib.rtc_render_filtered_rgb8(scene, C.byref(rc), C.byref(spc), C.byref(flc), 5, rgb8.ctypes.data, None) == 0, lib.rtc_last_error()
    assert lib.rtc_quantize(scene, np.ascontiguousarray(whole).ctypes.data, whole.size, q.ctypes.data) == 0, lib.rtc_last_error()
    assert np.array_equal(rgb8, q) and rgb8.max() > 0
    # the Python layers
    assert np.array_equal(bits(hip.render_filtered(nw, cam, sp, flt, 5)), bits(whole))
    assert np.array_equal(bits(hip.render_filtered(nw, cam, sp, flt, 5, row_first=5, n_rows=1)), bits(parts[1]))
    img = Image.par_render(cam, world, sampling=sp, filter=flt)
    assert (img.hsize, img.vsize) == (w, h) and np.array_equal(bits(np.asarray(img.pixels).reshape(-1, 3)), bits(whole))
    one = Image.par_render(cam, world, filter=Filter.tent(1.5))   # no sampling: one centre sample per pixel
    assert np.array_equal(bits(np.asarray(one.pixels).reshape(-1, 3)), bits(hip.render_filtered(nw, cam, Sampling(side=1), Filter.tent(1.5), 5)))
    # which branch of the gather kernel a frame takes, as the library reports it
    capfd.readouterr()
    monkeypatch.setenv("RTC_SAMPLED_TIMING", "1")
    filtered(lib, scene, cam, sp, flt, 5, stats=RtcStatsC())
    assert "(LDS, tile" in capfd.readouterr().err
    filtered(lib, scene, cam, sp, Filter.box(0.5), 5, stats=RtcStatsC())
    assert "(memory, tile" in capfd.readouterr().err


# ---- 6. stats ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("path", PATHS)
def test_stats_count_the_traced_rays(hip, path, monkeypatch):
    monkeypatch.setenv("RTC_KERNEL", path)
    monkeypatch.delenv("RTC_SAMPLED_MAX_RAYS", raising=False)
    lib = hip.lib
    name, (w, h), sp, flt = MITCHELL_CASE
    cam, world = getattr(scenes, name)(w, h)
    nw = hip.build_world(world)
    scene = lib.rtw_world_scene(nw.handle, 0)
    st = RtcStatsC()
    a = filtered(lib, scene, cam, sp, flt, 5, stats=st)
    assert st.pixels == w * h and st.rays_primary == w * h * 9 and st.kernel_ms > 0.0
    assert st.n_launches == (2 * 5 + 4 if path == "4" else 1) + 2     # one chunk: the trace launches, the generator and the filter kernel
    assert np.array_equal(bits(a), bits(filtered(lib, scene, cam, sp, flt, 5)))   # the counting kernels give the same pixels
    monkeypatch.setenv("RTC_SAMPLED_MAX_RAYS", "1")   # one output row per chunk, each with its halo inside the image
    W = window(flt.radius)
    traced = sum(min(h, y + W + 1) - max(0, y - W) for y in range(h))
    st1 = RtcStatsC()
    filtered(lib, scene, cam, sp, flt, 5, stats=st1)
    assert W == 2 and st1.pixels == w * h and st1.rays_primary == traced * w * 9 and st1.rays_primary > st.rays_primary
    st2 = RtcStatsC()
    filtered(lib, scene, cam, sp, flt, 5, 5, 1, stats=st2)
    assert st2.pixels == w and st2.rays_primary == 5 * w * 9   # one row of a range: its halo is traced though it is not returned


# ---- 7. path choice -----------------------------------------------------------------------------------------------------------------
def test_filtered_launches_choose_their_path(hip, monkeypatch):
    monkeypatch.delenv("RTC_KERNEL", raising=False)
    lib = hip.lib
    cam, world = scenes.chapter11_glass_air_bubble(64, 32)
    nw = hip.build_world(world)
    scene = lib.rtw_world_scene(nw.handle, 0)
    sp, flt = Sampling(side=2), Filter.tent(1.5)
    frames = [filtered(lib, scene, cam, sp, flt, 5) for _ in range(4)]
    ch, t1, t4 = C.c_int32(0), C.c_double(-1.0), C.c_double(-1.0)
    lib.rtc_scene_path_info(scene, C.byref(ch), C.byref(t1), C.byref(t4))
    assert ch.value in (1, 4) and t1.value > 0.0 and t4.value > 0.0, (ch.value, t1.value, t4.value)
    assert np.array_equal(bits(filtered(lib, scene, cam, sp, flt, 5)), bits(frames[0]))
    assert all(np.array_equal(bits(f), bits(frames[0])) for f in frames)
    # another filter or another row range is another launch shape: undecided again
    filtered(lib, scene, cam, sp, Filter.mitchell(2.0), 5)
    lib.rtc_scene_path_info(scene, C.byref(ch), C.byref(t1), C.byref(t4))
    assert ch.value == 0
