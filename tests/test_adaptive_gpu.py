"""Adaptive sampling (include/rtc.h rtc_adaptive) on an MI355X, both device paths.  Every pixel of an adaptive frame is, bit for bit, a
pixel of one of two rtc_render_sampled frames, chosen by the contrast rule on the first of them; so the checks are identities: the device's
compaction against the host evaluation of the same function (test_adaptive_cpu.py compares that with a numpy restatement), the two
degenerate thresholds against the two frames, and the general case against np.where(mask, fine frame, base frame) with the mask
restated in numpy from the device's own base frame.

The rule as restated (test_adaptive_cpu.contrast_mask): q(c) = 0 where c < 0, 1 where c > 1, else c; for a neighbour r of p inside the
image ((x+-1, y), (x, y+-1), with neighbours == 8 the diagonals too) d starts as |q(p[0]) - q(r[0])| and takes e = |q(p[c]) - q(r[c])|
for c = 1, 2 where e > d (a NaN first channel stays, a later NaN is skipped); p is refined iff some neighbour has not (d <= threshold)."""
import ctypes as C
import math

import numpy as np
import pytest

import foreign_flattener as ff
from raytracer_challenge_amd import scenes
from raytracer_challenge_amd.backend import AdaptiveC
from raytracer_challenge_amd.device import RtcStatsC
from raytracer_challenge_amd.image import Image
from raytracer_challenge_amd.scene import Adaptive, Sampling
from test_adaptive_cpu import SHAPES, THRESHOLDS, contrast_mask, random_frame
from test_sampled_camera_cpu import block_mean
from test_sampled_camera_gpu import bits, fine_frame, resized, scene_of

pytestmark = pytest.mark.gpu
PATHS = ["1", "4"]
vp = C.c_void_p
FINE = Sampling(side=4, jitter=True, seed=31)


def adaptive(lib, scene, cam, ad, fuel=5, stats=None):
    """rtc_render_adaptive through C: (frame, mask, n_refined)."""
    rc, adc = ff.make_camera(cam), AdaptiveC.of(ad)
    n = cam.hsize * cam.vsize
    rgb, mask, n_ref = np.full((n, 3), np.nan), np.full(n, 7, dtype=np.uint8), C.c_uint64(1 << 63)
    code = lib.rtc_render_adaptive(scene, C.byref(rc), C.byref(adc), fuel, rgb.ctypes.data, mask.ctypes.data, C.byref(n_ref), None if stats is None else C.byref(stats))
    assert code == 0, lib.rtc_last_error()
    assert set(np.unique(mask).tolist()) <= {0, 1}
    return rgb, mask.astype(bool), int(n_ref.value)


def setup(hip, name, w, h):
    """(lib, world handle, scene, camera) of a scene of `scenes` at w x h."""
    lib = hip.lib
    cam, world = getattr(scenes, name)(w, h)
    nw = hip.build_world(world)
    return lib, nw, lib.rtw_world_scene(nw.handle, 0), cam


def check_identity(hip, lib, nw, scene, cam, ad, label, share=(0.0, 1.0), stats=None):
    """The general case: mask, count and every pixel against the numpy rule on the device's own base frame.  Returns the mask."""
    n = cam.hsize * cam.vsize
    base, fine = hip.render_sampled(nw, cam, ad.base, 5), hip.render_sampled(nw, cam, ad.fine, 5)
    M = contrast_mask(base, cam.hsize, cam.vsize, ad.threshold, ad.neighbours)
    got, mask, n_ref = adaptive(lib, scene, cam, ad, stats=stats)
    print("%s: %d of %d pixels refined" % (label, int(M.sum()), n))
    assert np.array_equal(mask, M) and n_ref == int(M.sum()), (label, n_ref, int(M.sum()))
    assert np.array_equal(bits(got), bits(np.where(M[:, None], fine, base))), label
    assert share[0] * n <= M.sum() <= share[1] * n and 0 < M.sum() < n, (label, int(M.sum()), n)   # neither an empty nor a full mask
    return M


# ---- 1. the compaction alone: the device's list is the host evaluation's ------------------------------------------------------------
@pytest.mark.parametrize("path", PATHS)
def test_compaction_is_the_host_evaluation(hip, path, monkeypatch):
    monkeypatch.setenv("RTC_KERNEL", path)
    nw = hip.build_world(scenes.chapter11_glass_air_bubble(8, 8)[1])
    for hsize, vsize in SHAPES:
        frame = random_frame(hsize, vsize, 1000 + hsize)
        for neighbours in (4, 8):
            for threshold in THRESHOLDS:
                host = hip.contrast_pixels(frame, hsize, vsize, threshold, neighbours)
                dev = hip.contrast_pixels(frame, hsize, vsize, threshold, neighbours, nw=nw)
                assert dev.size == host.size and np.array_equal(dev, host), ((hsize, vsize), neighbours, threshold, dev.size, host.size)


@pytest.mark.parametrize("path", PATHS)
def test_compaction_over_more_blocks_than_one_scan_tile(hip, path, monkeypatch):
    """1024 x 1024: 4096 blocks of 256 pixels, 16 tiles of the scan's first level, one of its second."""
    monkeypatch.setenv("RTC_KERNEL", path)
    nw = hip.build_world(scenes.chapter11_glass_air_bubble(8, 8)[1])
    side, n = 1024, 1024 * 1024
    rng = np.random.default_rng(77)
    noise = rng.uniform(-0.5, 1.5, size=(n, 3))
    sparse = np.full((n, 3), 0.5)
    sparse[rng.choice(n, size=210, replace=False), 1] = 1.0   # each bright pixel refines itself and its (up to) four neighbours
    for label, frame, threshold, lo, hi in (("all", noise, -1.0, n, n), ("none", noise, math.inf, 0, 0), ("about 0.1 %", sparse, 0.25, 800, 1050)):
        host = hip.contrast_pixels(frame, side, side, threshold, 4)
        dev = hip.contrast_pixels(frame, side, side, threshold, 4, nw=nw)
        assert lo <= host.size <= hi, (label, host.size)
        assert dev.size == host.size and np.array_equal(dev, host), (label, dev.size, host.size)
    dev8 = hip.contrast_pixels(noise, side, side, 0.9, 8, nw=nw)   # a dense, irregular mask: every wave's popcount differs
    assert 0 < dev8.size < n and np.array_equal(dev8, hip.contrast_pixels(noise, side, side, 0.9, 8))


# ---- 2. the degenerate thresholds: the two frames themselves ---------------------------------------------------------------------------
@pytest.mark.parametrize("name,w,h", [("cover", 48, 32), ("chapter11_title", 37, 19)])
@pytest.mark.parametrize("path", PATHS)
def test_threshold_inf_is_the_base_frame(hip, path, name, w, h, monkeypatch):
    monkeypatch.setenv("RTC_KERNEL", path)
    lib, nw, scene, cam = setup(hip, name, w, h)
    for base in (Sampling(), Sampling(side=2, jitter=True, seed=3)):
        got, mask, n_ref = adaptive(lib, scene, cam, Adaptive(base, FINE, math.inf))
        assert n_ref == 0 and not mask.any()
        assert np.array_equal(bits(got), bits(hip.render_sampled(nw, cam, base, 5))), (name, base)
    assert np.array_equal(bits(adaptive(lib, scene, cam, Adaptive(Sampling(), FINE, math.inf))[0]), bits(hip.render(nw, cam, 5, want_hits=False)[0]))


@pytest.mark.parametrize("name,w,h", [("cover", 48, 32), ("chapter11_title", 37, 19)])
@pytest.mark.parametrize("path", PATHS)
def test_negative_threshold_is_the_fine_frame(hip, path, name, w, h, monkeypatch):
    monkeypatch.setenv("RTC_KERNEL", path)
    lib, nw, scene, cam = setup(hip, name, w, h)
    for fine in (Sampling(side=2), Sampling(side=3, jitter=True, seed=4), Sampling(side=4, jitter=True, seed=5, lens_radius=0.1, focal_distance=5.0)):
        got, mask, n_ref = adaptive(lib, scene, cam, Adaptive(Sampling(), fine, -1.0))
        assert n_ref == w * h and mask.all()
        assert np.array_equal(bits(got), bits(hip.render_sampled(nw, cam, fine, 5))), (name, fine)


# ---- 3. the general case ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,threshold", [("cover", 0.1), ("chapter11_title", 0.3)])
@pytest.mark.parametrize("path", PATHS)
def test_general_case_is_np_where_of_the_two_frames(hip, path, name, threshold, monkeypatch):
    """The oracle's renders of these frames refine 702 (4 neighbours) / 828 (8) of cover's 1536 pixels at 0.1 and 161 / 232 of
    chapter11_title's at 0.3; the share is asserted within [5 %, 95 %]."""
    monkeypatch.setenv("RTC_KERNEL", path)
    lib, nw, scene, cam = setup(hip, name, 48, 32)
    for neighbours in (4, 8):
        st = RtcStatsC()
        M = check_identity(hip, lib, nw, scene, cam, Adaptive(Sampling(), FINE, threshold, neighbours), "%s path %s, %d neighbours" % (name, path, neighbours),
                           share=(0.05, 0.95), stats=st)
        assert st.pixels == 1536 and st.rays_primary == 1536 + 16 * int(M.sum()) and st.kernel_ms > 0.0
        got, mask, n_ref = adaptive(lib, scene, cam, Adaptive(Sampling(), FINE, threshold, neighbours))   # without counters: the plain kernel variants
        assert np.array_equal(mask, M) and np.array_equal(bits(got), bits(np.where(M[:, None], hip.render_sampled(nw, cam, FINE, 5), hip.render(nw, cam, 5, want_hits=False)[0])))


_coarse = {}


@pytest.mark.parametrize("path", PATHS)
def test_against_the_oracle(hip, orc, path, monkeypatch):
    """With the device's mask: refined pixels are the 2x2 block means of the oracle's 96x64 frame (an unjittered 2x2 grid is the finer
    camera's pixel set, test_sampled_camera_cpu.py), the others the oracle's 48x32 pixels; 1e-5 is the project's colour tolerance."""
    monkeypatch.setenv("RTC_KERNEL", path)
    lib, nw, scene, cam = setup(hip, "cover", 48, 32)
    if "cover" not in _coarse:
        _coarse["cover"] = orc.render(orc.build_world(scenes.cover(48, 32)[1]), cam, 5)[0]
    got, mask, n_ref = adaptive(lib, scene, cam, Adaptive(Sampling(), Sampling(side=2), 0.1))
    assert 0.05 * 1536 <= n_ref <= 0.95 * 1536
    want = np.where(mask[:, None], block_mean(fine_frame(orc, "cover"), 48, 32, 2), _coarse["cover"])
    err = float(np.abs(got - want).max())
    print("cover path %s: %d pixels refined, max |dRGB| vs the oracle's frames = %.3e" % (path, n_ref, err))
    assert err <= 1e-5, err


# ---- 4. every scene kind through the refine pass -----------------------------------------------------------------------------------
KINDS = {  # scene -> (frame, threshold): thresholds at which the base frame has both flat regions and edges (8 neighbours: the CPU
    # emulator's base frames refine 230 of 384, 115 of 384 and 181 of 703 pixels of the three scenes it can render)
    "csg_scene": ((24, 16), 0.5),
    "teapot_low": ((24, 16), 0.1),
    "area_light_jittered": ((24, 16), 0.05),
    "texture_showcase": ((24, 16), 0.3),
    "glass_and_mirrors": ((37, 19), 0.5),
}


@pytest.mark.parametrize("name", sorted(KINDS))
@pytest.mark.parametrize("path", PATHS)
def test_scene_kinds_through_the_refine_pass(hip, path, name, monkeypatch):
    monkeypatch.setenv("RTC_KERNEL", path)
    lib = hip.lib
    (w, h), threshold = KINDS[name]
    cam0, world = scenes.chapter11_glass_air_bubble(w, h) if name == "glass_and_mirrors" else scene_of(name)
    cam = resized(cam0, w, h)
    nw = hip.build_world(world)
    scene = lib.rtw_world_scene(nw.handle, 0)
    check_identity(hip, lib, nw, scene, cam, Adaptive(Sampling(), Sampling(side=3, jitter=True, seed=6), threshold, 8), "%s path %s" % (name, path))


# ---- 5. chunks, routes and buffer reuse change no bit -------------------------------------------------------------------------------
@pytest.mark.parametrize("path", PATHS)
def test_chunks_change_no_bit(hip, path, monkeypatch):
    monkeypatch.setenv("RTC_KERNEL", path)
    lib, nw, scene, cam = setup(hip, "chapter11_glass_air_bubble", 37, 19)
    for ad in (Adaptive(Sampling(), Sampling(side=3, jitter=True, seed=11), 0.5), Adaptive(Sampling(side=2, jitter=True, seed=12), Sampling(side=4, seed=13), 0.5, 8)):
        monkeypatch.delenv("RTC_SAMPLED_MAX_RAYS", raising=False)
        whole, mask, n_ref = adaptive(lib, scene, cam, ad)
        assert 0 < n_ref < 703
        for limit in ("1000", "1"):   # some refined pixels per chunk; one refined pixel (and one row of the sampled base pass) per chunk
            monkeypatch.setenv("RTC_SAMPLED_MAX_RAYS", limit)
            st = RtcStatsC()
            got, mask2, n2 = adaptive(lib, scene, cam, ad, stats=st)
            assert n2 == n_ref and np.array_equal(mask2, mask) and np.array_equal(bits(got), bits(whole)), limit
            assert st.pixels == 703 and st.rays_primary == 703 * ad.base.samples + n_ref * ad.fine.samples
            if limit == "1000":
                assert np.array_equal(bits(adaptive(lib, scene, cam, ad)[0]), bits(whole))


@pytest.mark.parametrize("path", PATHS)
def test_other_routes_and_buffer_reuse(hip, path, monkeypatch):
    monkeypatch.setenv("RTC_KERNEL", path)
    lib, nw, scene, cam = setup(hip, "cover", 48, 32)
    ad = Adaptive(Sampling(), FINE, 0.1)
    whole, mask, n_ref = adaptive(lib, scene, cam, ad)
    assert 0 < n_ref < 1536
    # two consecutive calls on one scene: the buffers are reused
    again, mask2, n2 = adaptive(lib, scene, cam, ad)
    assert n2 == n_ref and np.array_equal(mask2, mask) and np.array_equal(bits(again), bits(whole))
    # a smaller frame after a larger one is the smaller frame's own render (a fresh scene renders it alone)
    small_cam = resized(cam, 21, 13)
    small, small_mask, small_n = adaptive(lib, scene, small_cam, ad)
    nw2 = hip.build_world(scenes.cover(21, 13)[1])
    alone, alone_mask, alone_n = adaptive(lib, lib.rtw_world_scene(nw2.handle, 0), small_cam, ad)
    assert small_n == alone_n and 0 < small_n < 273 and np.array_equal(small_mask, alone_mask) and np.array_equal(bits(small), bits(alone))
    assert np.array_equal(bits(adaptive(lib, scene, cam, ad)[0]), bits(whole))   # and the larger one again
    # quantised on the device
    rc, adc = ff.make_camera(cam), AdaptiveC.of(ad)
    rgb8, q, mask8, n8 = np.zeros(whole.size, dtype=np.uint8), np.zeros(whole.size, dtype=np.uint8), np.full(1536, 7, dtype=np.uint8), C.c_uint64(0)
    assert lib.rtc_render_adaptive_rgb8(scene, C.byref(rc), C.byref(adc), 5, rgb8.ctypes.data, mask8.ctypes.data, C.byref(n8), None) == 0, lib.rtc_last_error()
    assert lib.rtc_quantize(scene, np.ascontiguousarray(whole).ctypes.data, whole.size, q.ctypes.data) == 0, lib.rtc_last_error()
    assert np.array_equal(rgb8, q) and rgb8.max() > 0 and n8.value == n_ref and np.array_equal(mask8.astype(bool), mask)
    # the outputs a caller does not want
    assert lib.rtc_render_adaptive(scene, C.byref(rc), C.byref(adc), 5, again.ctypes.data, None, None, None) == 0 and np.array_equal(bits(again), bits(whole))
    # the Python layers
    rgb_py, mask_py = hip.render_adaptive(nw, cam, ad, 5, want_mask=True)
    assert np.array_equal(bits(rgb_py), bits(whole)) and mask_py.dtype == bool and np.array_equal(mask_py, mask)
    assert np.array_equal(bits(hip.render_adaptive(nw, cam, ad, 5)), bits(whole))
    img = Image.par_render(cam, scenes.cover(48, 32)[1], adaptive=ad)
    assert (img.hsize, img.vsize) == (48, 32) and np.array_equal(bits(np.asarray(img.pixels).reshape(-1, 3)), bits(whole))


# ---- 6. the compaction past 2^24 pixels: three scan levels ---------------------------------------------------------------------------
WIDE = (4096, 4097)   # 16 781 312 pixels in 65 552 blocks: block counts -> 257 tile sums -> 2 -> 1, one entry past a tile at the second level
WIDE_PLANTED = (0, 255, 256, 65535, 65536, (1 << 24) - 1, 1 << 24, 4096 * 4097 - 1,   # the seams of the first and second level, 2^24, the last pixel
                5000, 5001,                    # pairs that touch: in a row,
                9000000, 9000000 + 4096,       #   in a column,
                12345678, 12345678 + 4097)     #   across a corner


@pytest.fixture(scope="module")
def wide(hip):
    """(the frame: 0.5 everywhere but the planted pixels' green, a scene to compact it on); the frame is 403 MB on the host and on the device
    and the list 134 MB more, so the scene is released when the module is done."""
    w, h = WIDE
    frame = np.full((w * h, 3), 0.5)
    frame[np.array(WIDE_PLANTED), 1] = 1.0
    nw = hip.build_world(scenes.chapter11_glass_air_bubble(8, 8)[1])
    yield frame, nw
    nw.close()


def planted_and_neighbours(planted, w, h, neighbours):
    """The sorted union of the planted pixels and their neighbours inside the frame, from the planted set alone."""
    p = np.array(planted, dtype=np.int64)
    x, y = p % w, p // w
    steps = [(-1, 0), (1, 0), (0, -1), (0, 1)] + ([(-1, -1), (1, -1), (-1, 1), (1, 1)] if neighbours == 8 else [])
    out = [p]
    for dx, dy in steps:
        inside = (x + dx >= 0) & (x + dx < w) & (y + dy >= 0) & (y + dy < h)
        out.append(((y + dy) * w + (x + dx))[inside])
    return np.unique(np.concatenate(out)).astype(np.uint64)


@pytest.mark.parametrize("neighbours", [4, 8])
def test_compaction_of_a_sparse_frame_past_2_to_24_pixels(hip, wide, neighbours):
    """A bright pixel differs by 0.5 from every dark neighbour and by 0 from a bright one, and none is surrounded by bright ones: at 0.25
    the refined pixels are the planted ones and their neighbours."""
    frame, nw = wide
    w, h = WIDE
    want = planted_and_neighbours(WIDE_PLANTED, w, h, neighbours)
    assert want.size < len(WIDE_PLANTED) * (neighbours + 1) and int(want[-1]) == w * h - 1 and int(want[0]) == 0
    host = hip.contrast_pixels(frame, w, h, 0.25, neighbours)
    assert host.size == want.size and np.array_equal(host, want), (host.size, want.size)
    dev = hip.contrast_pixels(frame, w, h, 0.25, neighbours, nw=nw)
    assert dev.size == want.size and np.array_equal(dev, want), (dev.size, want.size, dev[:40], want[:40])


def test_compaction_of_every_pixel_past_2_to_24_pixels(hip, wide):
    """Threshold -1 refines every pixel: every block count is 256 and the prefix sums reach 16.8 M."""
    frame, nw = wide
    w, h = WIDE
    dev = hip.contrast_pixels(frame, w, h, -1.0, 4, nw=nw)
    assert dev.size == w * h
    bad = np.flatnonzero(dev != np.arange(w * h, dtype=np.uint64))
    assert bad.size == 0, "%d entries are not their own index, the first at %d" % (bad.size, int(bad[0]))
    # and a small frame afterwards, in the grown buffers
    small = random_frame(13, 7, 5)
    assert np.array_equal(hip.contrast_pixels(small, 13, 7, 0.3, 8, nw=nw), hip.contrast_pixels(small, 13, 7, 0.3, 8))
