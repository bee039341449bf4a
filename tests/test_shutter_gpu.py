"""The shutter (include/rtc.h rtc_shutter) on an MI355X, both device paths.  The oracle and the emulator know nothing of it, so the
semantics are pinned through the definition itself: the device's dealing is the host evaluation's (test_shutter_cpu.py compares that
with a restatement); K = 1 and K equal poses are rtc_render_sampled's frame; a frame over different poses is, bit for bit, the k-ordered
mean of rtc_trace_rays over the host's sample rays of the pose each sample is dealt to; chunks, the quantiser, the counters and the
Python layer change no bit; a sphere crossing the frame leaves the mean of its still frames."""
import ctypes as C
import math

import numpy as np
import pytest

import ext_cases
from raytracer_challenge_amd import scenes
from raytracer_challenge_amd.backend import HIT_DTYPE
from raytracer_challenge_amd.device import RtcCameraC, RtcStatsC
from raytracer_challenge_amd.image import Image
from raytracer_challenge_amd.scene import Camera, Color, Element, Material, Matrix, Pattern, PointLight, Sampling, ShapeArgs, Shutter, Vector, World
from test_sampled_camera_cpu import samples_mean
from test_shutter_cpu import BIG_DEALS, FRAME, LIST7, big_deal_case, check_dealing_properties, poses_np, poses_of

pytestmark = pytest.mark.gpu
PATHS = ["1", "4"]
vp = C.c_void_p


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def trace(lib, nw, rays, fuel, stats=None):
    """rtc_trace_rays on a world's scene: the colours of the rays (rows {o, d})."""
    rays = np.ascontiguousarray(rays, dtype=np.float64).reshape(-1, 6)
    rgb, hits = np.full((rays.shape[0], 3), np.nan), np.empty(rays.shape[0], dtype=HIT_DTYPE)
    code = lib.rtc_trace_rays(lib.rtw_world_scene(nw.handle, 0), rays.ctypes.data, rays.shape[0], fuel, rgb.ctypes.data, hits.ctypes.data,
                              None if stats is None else C.byref(stats))
    assert code == 0, lib.rtc_last_error()
    return rgb


def expected_frame(hip, lib, nws, cams, sp, shutter, fuel, pixels, shadow=None):
    """The definition, outside the library's shutter code: host sample rays per pose camera, the restated pose picks each sample's row,
    rtc_trace_rays on that pose's scene, the k-ordered sum / N in numpy.  shadow: a list that receives each pose's rays_shadow."""
    K, N = len(nws), sp.samples
    if len(pixels) * N > 100000:   # (the Python-int restatement is for small frames; test_shutter_cpu.py holds the two to one answer)
        pose = poses_np(sp, shutter.hashed, K, pixels).reshape(len(pixels), N)
    else:
        pose = poses_of(sp, shutter.hashed, K, [int(i) for i in pixels]).reshape(len(pixels), N)
    colours = np.full((len(pixels), N, 3), np.nan)
    host_rays = []   # (camera, its rays): evaluated once per distinct camera object, not once per pose
    for p in range(K):
        sel = pose == p
        if not sel.any():
            continue
        rays = next((r for c, r in host_rays if c is cams[p]), None)
        if rays is None:
            rays = hip.camera_rays(cams[p], sp, pixel_indices=np.asarray(pixels, dtype=np.uint64))    # host evaluation: no world
            host_rays.append((cams[p], rays))
        st = RtcStatsC()
        colours[sel] = trace(lib, nws[p], rays[sel], fuel, stats=st)
        if shadow is not None:
            shadow.append(int(st.rays_shadow))
    return samples_mean(colours)


# ---- 1. the device's dealing is the host evaluation's ----------------------------------------------------------------------------------
DEALS = [  # (K, hashed, side, a pixel list or None for the whole 37x19 frame)
    (3, True, 3, None),        # 6 327 samples: neither a multiple of 64 nor of 256, 25 blocks
    (64, True, 3, None),       # many poses per wave
    (2, False, 16, None),      # whole waves of one pose
    (5, False, 3, None),       # runs of 1 and 2 samples
    (64, True, 1, LIST7),      # 7 samples: at least 57 empty poses
    (1, True, 3, None),
    (1, False, 1, LIST7),
]


@pytest.mark.parametrize("K,hashed,side,pixels", DEALS)
def test_device_dealing_is_the_host_dealing(hip, K, hashed, side, pixels):
    _, world = scenes.chapter11_glass_air_bubble(*FRAME)
    nw = hip.build_world(world)
    sp, sh = Sampling(side=side, seed=1234 + K), Shutter(hashed)
    kw = dict(n=FRAME[0] * FRAME[1]) if pixels is None else dict(pixel_indices=pixels)
    dev, host = hip.shutter_deal(FRAME[0], K, sp, sh, nw=nw, **kw), hip.shutter_deal(FRAME[0], K, sp, sh, **kw)
    assert np.array_equal(dev[1], host[1]), (dev[1], host[1])
    assert np.array_equal(dev[0], host[0])
    if pixels is not None and K == 64:
        assert int((np.diff(dev[1].astype(np.int64)) == 0).sum()) >= 57
    # a smaller dealing after a larger one reuses the buffers; a range that is not whole rows is a list launch
    dev2, host2 = hip.shutter_deal(FRAME[0], K, sp, sh, nw=nw, first=5, n=40), hip.shutter_deal(FRAME[0], K, sp, sh, first=5, n=40)
    assert np.array_equal(dev2[0], host2[0]) and np.array_equal(dev2[1], host2[1])


# ---- 1b. the dealing of a production chunk: count tables of two full scan levels, and of three ------------------------------------------------
BIG_DEVICE_DEALS = [d + (False,) for d in BIG_DEALS] + [  # (hsize, vsize, side, K, hashed, as a pixel list)
    (512, 512, 4, 4, True, False),       # 65 536 entries: exactly two full levels
    (512, 512, 4, 64, True, False),      # 2^20 entries
    (128, 129, 4, 64, True, True),       # the frame as a list: a permutation with a few indices repeated
]


def listed_frame(hsize, vsize):
    px = np.random.default_rng(hsize * vsize).permutation(hsize * vsize).astype(np.uint64)
    px[[5, 300, 9000, px.size - 1]] = px[[4, 299, 17, 0]]   # four pixels twice (and four not at all)
    return px


@pytest.mark.parametrize("hsize,vsize,side,K,hashed,listed", BIG_DEVICE_DEALS)
def test_device_dealing_of_a_production_chunk(hip, hsize, vsize, side, K, hashed, listed):
    _, world = scenes.chapter11_glass_air_bubble(*FRAME)
    nw = hip.build_world(world)
    pixels = listed_frame(hsize, vsize) if listed else None
    sp, sh, poses, (want_order, want_offsets) = big_deal_case(hsize, vsize, side, K, hashed, pixels)
    kw = dict(pixel_indices=pixels) if listed else dict(n=hsize * vsize)
    dev, host = hip.shutter_deal(hsize, K, sp, sh, nw=nw, **kw), hip.shutter_deal(hsize, K, sp, sh, **kw)
    assert np.array_equal(dev[1], want_offsets) and np.array_equal(host[1], want_offsets), (dev[1], host[1], want_offsets)
    bad = np.flatnonzero(dev[0] != want_order)
    assert bad.size == 0, "%d of %d positions differ from the restated dealing, the first at %d" % (bad.size, want_order.size, int(bad[0]))
    assert np.array_equal(host[0], want_order)
    check_dealing_properties(dev[0], dev[1], poses, K)
    # the small dealings of test_device_dealing_is_the_host_dealing on the same scene: the grown buffers are reused
    sp2, sh2 = Sampling(side=3, seed=1237), Shutter()
    for kw2 in (dict(n=FRAME[0] * FRAME[1]), dict(first=5, n=40)):
        dev2, host2 = hip.shutter_deal(FRAME[0], 3, sp2, sh2, nw=nw, **kw2), hip.shutter_deal(FRAME[0], 3, sp2, sh2, **kw2)
        assert np.array_equal(dev2[0], host2[0]) and np.array_equal(dev2[1], host2[1])


# ---- 2. identities with rtc_render_sampled -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hashed", [False, True])
@pytest.mark.parametrize("path", PATHS)
def test_one_pose_and_equal_poses_are_rtc_render_sampled(hip, path, hashed, monkeypatch):
    monkeypatch.setenv("RTC_KERNEL", path)
    cam, world = scenes.chapter11_glass_air_bubble(*FRAME)
    nw, twin = hip.build_world(world), hip.build_world(scenes.chapter11_glass_air_bubble(*FRAME)[1])   # equal scenes created twice
    sp, sh = Sampling(side=3, jitter=True, seed=17, lens_radius=0.15, focal_distance=5.0), Shutter(hashed)
    want = hip.render_sampled(nw, cam, sp, 5)
    assert np.isfinite(want).all() and want.max() > 0.0
    assert np.array_equal(bits(hip.render_shutter([nw], [cam], sp, sh, 5)), bits(want))
    assert np.array_equal(bits(hip.render_shutter([nw] * 5, [cam] * 5, sp, sh, 5)), bits(want))                   # the same pointer five times
    assert np.array_equal(bits(hip.render_shutter([nw, twin, twin, nw, twin], [cam] * 5, sp, sh, 5)), bits(want))  # two scenes, mixed
    assert np.array_equal(bits(hip.render_shutter([twin, nw, nw], [cam] * 3, sp, sh, 5, pixel_indices=LIST7)), bits(want[LIST7.astype(np.int64)]))


# ---- 3. the general case ---------------------------------------------------------------------------------------------------------------
_general = {}


def general(hip):
    """The three poses of the motion scene, built once."""
    if not _general:
        poses = scenes.motion_showcase(FRAME[0], FRAME[1], 3)
        _general["cams"] = [c for c, _ in poses]
        _general["worlds"] = [w for _, w in poses]
    return _general["cams"], [hip.build_world(w) for w in _general["worlds"]]   # (scenes are created under the test's RTC_KERNEL)


@pytest.mark.parametrize("path", PATHS)
def test_a_frame_is_the_mean_of_its_samples_each_in_its_pose(hip, path, monkeypatch):
    monkeypatch.setenv("RTC_KERNEL", path)
    lib = hip.lib
    cams, nws = general(hip)
    sp, sh = Sampling(side=3, jitter=True, seed=29), Shutter()
    pixels = np.arange(FRAME[0] * FRAME[1], dtype=np.uint64)
    key = ("want", sp, sh)
    if key not in _general:   # (computed under the first path, shared: the other path must give these bits too)
        _general[key] = expected_frame(hip, lib, nws, cams, sp, sh, 5, pixels)
    want = _general[key]
    assert np.isfinite(want).all() and want.max() > 0.0
    got = hip.render_shutter(nws, cams, sp, sh, 5)
    assert np.array_equal(bits(got), bits(want))
    # the poses differ: no still frame is this frame
    assert all(not np.array_equal(bits(hip.render_sampled(nws[p], cams[p], sp, 5)), bits(got)) for p in range(3))
    # a pixel list with a repeated index
    listed = hip.render_shutter(nws, cams, sp, sh, 5, pixel_indices=LIST7)
    assert np.array_equal(bits(listed), bits(want[LIST7.astype(np.int64)]))
    assert np.array_equal(bits(listed), bits(expected_frame(hip, lib, nws, cams, sp, sh, 5, LIST7)))
    # sequential mode over the same poses
    seq = Shutter(hashed=False)
    assert np.array_equal(bits(hip.render_shutter(nws, cams, sp, seq, 5, pixel_indices=LIST7)), bits(expected_frame(hip, lib, nws, cams, sp, seq, 5, LIST7)))


# ---- 3b. a frame across a dealing of three scan levels ----------------------------------------------------------------------------------------
_wide = {}


@pytest.mark.parametrize("path", PATHS)
def test_a_frame_across_a_three_level_dealing(hip, path, monkeypatch):
    """128x129 at 4x4 jittered samples over K = 64 hashed poses, one default chunk: 264 192 samples in 1 032 blocks, a count table of
    66 048 entries -> 258 -> 2: two entries past a tile at the second level, so the table from entry 65 536 on -- pose 63's blocks
    520 .. 1 031 -- gets its base from the third level, which no offset shows."""
    monkeypatch.setenv("RTC_KERNEL", path)
    monkeypatch.delenv("RTC_SAMPLED_MAX_RAYS", raising=False)
    lib = hip.lib
    W, H, K = 128, 129, 64
    cam, world = scenes.chapter11_glass_air_bubble(W, H)
    nw, twin = hip.build_world(world), hip.build_world(scenes.chapter11_glass_air_bubble(W, H)[1])
    sp, sh = Sampling(side=4, jitter=True, seed=41), Shutter()
    # identity: one camera 64 times over two equal scenes
    still = hip.render_sampled(nw, cam, sp, 5)
    assert np.isfinite(still).all() and still.max() > 0.0
    assert np.array_equal(bits(hip.render_shutter([nw, twin] * 32, [cam] * K, sp, sh, 5)), bits(still))
    # definition: two cameras alternate over the poses
    cam2 = Camera.new(W, H, math.pi / 3.0, Camera.transform(Vector.point(0.4, 2.5, 0.2), Vector.point(0.0, 0.0, 0.0), Vector.vector(0.0, 0.0, 1.0)))
    nws, cams = [nw, twin] * 32, [cam, cam2] * 32
    if "want" not in _wide:   # (computed under the first path, shared: the other path must give these bits too)
        _wide["want"] = expected_frame(hip, lib, nws, cams, sp, sh, 5, np.arange(W * H, dtype=np.uint64))
    want = _wide["want"]
    assert np.isfinite(want).all() and want.max() > 0.0
    st = RtcStatsC()
    got = hip.render_shutter(nws, cams, sp, sh, 5, stats=st)
    assert np.array_equal(bits(got), bits(want))
    assert not np.array_equal(bits(got), bits(still))
    assert np.array_equal(bits(hip.render_shutter(nws, cams, sp, sh, 5)), bits(want))     # without counters: the plain kernel builds
    T = 2 * 5 + 4 if path == "4" else 1    # trace launches of one run
    assert st.pixels == W * H and st.rays_primary == 16512 * 16
    # one chunk: count, three scan levels up and two down, place; per pose (none is empty) a generator and the traces; the resolve
    assert st.n_launches == 2 + (2 * 3 - 1) + K * (1 + T) + 1, st.n_launches


# ---- 4. chunks change no bit; 5. the quantised frame; 6. the counters ----------------------------------------------------------------
@pytest.mark.parametrize("path", PATHS)
def test_chunks_quantiser_and_counters(hip, path, monkeypatch):
    monkeypatch.setenv("RTC_KERNEL", path)
    lib = hip.lib
    cams, nws = general(hip)
    sp, sh = Sampling(side=3, jitter=True, seed=29), Shutter()
    whole = hip.render_shutter(nws, cams, sp, sh, 5)
    T = 2 * 5 + 4 if path == "4" else 1    # trace launches of one run
    st = RtcStatsC()
    assert np.array_equal(bits(hip.render_shutter(nws, cams, sp, sh, 5, stats=st)), bits(whole))   # the counting kernels give the same pixels
    shadow = []
    expected_frame(hip, lib, nws, cams, sp, sh, 5, np.arange(703, dtype=np.uint64), shadow=shadow)
    assert st.pixels == 703 and st.rays_primary == 703 * 9 and st.kernel_ms > 0.0
    assert len(shadow) == 3 and st.rays_shadow == sum(shadow) > 0
    assert st.n_launches == 3 + 3 * (1 + T) + 1     # one chunk: count, one scan level, place; per pose a generator and the traces; the resolve
    st7 = RtcStatsC()
    hip.render_shutter(nws, cams, sp, sh, 5, pixel_indices=LIST7, stats=st7)
    assert st7.pixels == 7 and st7.rays_primary == 63
    # quantised on the device
    scene_p = (vp * 3)(*[lib.rtw_world_scene(nw.handle, 0) for nw in nws])
    cams_c = (RtcCameraC * 3)()
    for p, cam in enumerate(cams):
        cc = hip.camera_c(cam)
        assert lib.rtw_make_camera(C.byref(cc), C.byref(cams_c[p])) == 0
    from raytracer_challenge_amd.backend import SamplingC, ShutterC
    spc, shc = SamplingC.of(sp), ShutterC.of(sh)
    rgb8, q = np.zeros(whole.size, dtype=np.uint8), np.zeros(whole.size, dtype=np.uint8)
    assert lib.rtc_render_shutter_rgb8(scene_p, cams_c, 3, C.byref(shc), C.byref(spc), 5, rgb8.ctypes.data, None) == 0, lib.rtc_last_error()
    assert lib.rtc_quantize(scene_p[0], np.ascontiguousarray(whole).ctypes.data, whole.size, q.ctypes.data) == 0, lib.rtc_last_error()
    assert np.array_equal(rgb8, q) and rgb8.max() > 0
    # chunks
    monkeypatch.setenv("RTC_SAMPLED_MAX_RAYS", "1000")   # 3 rows of 333 rays per chunk: 7 chunks; 111 listed pixels per chunk
    st = RtcStatsC()
    assert np.array_equal(bits(hip.render_shutter(nws, cams, sp, sh, 5, stats=st)), bits(whole))
    assert st.pixels == 703 and st.rays_primary == 703 * 9 and st.rays_shadow == sum(shadow)
    assert np.array_equal(bits(hip.render_shutter(nws, cams, sp, sh, 5)), bits(whole))
    idx = np.arange(702, 2, -3, dtype=np.uint64)         # 234 pixels: 3 chunks
    assert np.array_equal(bits(hip.render_shutter(nws, cams, sp, sh, 5, pixel_indices=idx)), bits(whole[idx.astype(np.int64)]))
    monkeypatch.setenv("RTC_SAMPLED_MAX_RAYS", "1")      # never fewer than one row / one pixel
    assert np.array_equal(bits(hip.render_shutter(nws, cams, sp, sh, 5, pixel_indices=idx[:5])), bits(whole[idx[:5].astype(np.int64)]))


# ---- 7. every scene kind goes through ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("path", PATHS)
def test_a_scene_with_every_extension_goes_through(hip, path, monkeypatch):
    monkeypatch.setenv("RTC_KERNEL", path)
    world = ext_cases.everything_world()
    cam = ext_cases.everything_camera(24, 16)
    nw, twin = hip.build_world(world), hip.build_world(ext_cases.everything_world())
    sp = Sampling(side=2, jitter=True, seed=5)
    want = hip.render_sampled(nw, cam, sp, 5)
    assert np.isfinite(want).all() and want.max() > 0.0
    for sh in (Shutter(), Shutter(hashed=False)):
        assert np.array_equal(bits(hip.render_shutter([nw, twin], [cam, cam], sp, sh, 5)), bits(want))
    # and over two different cameras it is the definition
    lib = hip.lib
    cam2 = Camera.new(24, 16, 1.0, Camera.transform(Vector.point(0.5, 2.6, -7.0), Vector.point(-0.2, 0.8, 0.0), Vector.vector(0.0, 1.0, 0.0)))
    got = hip.render_shutter([nw, twin], [cam, cam2], sp, Shutter(), 5)
    assert np.array_equal(bits(got), bits(expected_frame(hip, lib, [nw, twin], [cam, cam2], sp, Shutter(), 5, np.arange(24 * 16, dtype=np.uint64))))
    assert not np.array_equal(bits(got), bits(want))


# ---- 8. the Python layer -------------------------------------------------------------------------------------------------------------
def test_par_render_shutter_is_the_c_call_and_builds_a_world_once(hip, monkeypatch):
    poses = scenes.motion_showcase(FRAME[0], FRAME[1], 3)
    world = poses[1][1]
    panning = [(c, world) for c, _ in poses]    # a moving camera over one static world
    sp = Sampling(side=2, jitter=True, seed=3)
    nw = hip.build_world(world)
    want = hip.render_shutter([nw] * 3, [c for c, _ in poses], sp, Shutter(), 5)
    built = []
    real = hip.build_world
    monkeypatch.setattr(hip, "build_world", lambda w: built.append(w) or real(w))
    img = Image.par_render_shutter(panning, sp, backend=hip)
    assert len(built) == 1 and built[0] is world
    assert (img.hsize, img.vsize) == FRAME and np.array_equal(bits(np.asarray(img.pixels).reshape(-1, 3)), bits(want))
    del built[:]
    img2 = Image.par_render_shutter(poses, sp, shutter=Shutter(hashed=False), backend=hip)
    assert len(built) == 3
    nws = [real(w) for _, w in poses]
    assert np.array_equal(bits(img2.pixels), bits(hip.render_shutter(nws, [c for c, _ in poses], sp, Shutter(hashed=False), 5)))
    assert img2.quantized().shape == (703, 3)


# ---- a physical check: a box shutter averages the still frames -----------------------------------------------------------------------------
def test_a_crossing_sphere_leaves_the_mean_of_its_still_frames(hip):
    """64x48, side 4, K = 8 hashed: a white sphere lit by its ambient term alone crosses a black background.  Every sample draws its
    pose independently and uniformly, so the frame's mean has expectation E = the mean over the poses of the still frames' means and
    variance sum over the samples of Var_p(c(sample, p)) / (P N)^2, computed here from the per-pose sample colours.  Bound: 6 standard errors."""
    K, N = 8, 16
    cam = Camera.new(64, 48, 1.0, Camera.transform(Vector.point(0.0, 0.0, -6.0), Vector.point(0.0, 0.0, 0.0), Vector.vector(0.0, 1.0, 0.0)))
    white = Material(pattern=Pattern.plain(Color(1.0, 1.0, 1.0)), ambient=1.0, diffuse=0.0, specular=0.0)
    light = PointLight(Color(1.0, 1.0, 1.0), Vector.point(0.0, 10.0, -10.0))
    worlds = [World([light], [Element.sphere(ShapeArgs(transform=Matrix.translation(-2.0 + 4.0 * p / (K - 1), 0.0, 0.0), material=white))]) for p in range(K)]
    nws = [hip.build_world(w) for w in worlds]
    sp = Sampling(side=4, jitter=True, seed=99)
    lib = hip.lib
    rays = hip.camera_rays(cam, sp)
    still = np.stack([trace(lib, nw, rays, 5)[:, 0].reshape(-1, N) for nw in nws])     # [K, pixels, N], channel 0
    still_frames = np.stack([hip.render_sampled(nw, cam, sp, 5)[:, 0] for nw in nws])
    assert 0.02 < still_frames.mean() < 0.5 and float(np.abs(still.mean(axis=2) - still_frames).max()) <= 1e-12
    expect = float(np.mean([f.mean() for f in still_frames]))
    se = math.sqrt(float(still.var(axis=0).sum())) / float(still.shape[1] * N)
    got = hip.render_shutter(nws, [cam] * K, sp, Shutter(), 5)
    mean = float(got[:, 0].mean())
    print("mean %.6f, expected %.6f, standard error %.3e: %.2f sigma" % (mean, expect, se, abs(mean - expect) / se))
    assert se > 0.0 and abs(mean - expect) <= 6.0 * se
    # blurred: pixels the sphere sweeps over are neither black nor white
    assert int(((got[:, 0] > 0.05) & (got[:, 0] < 0.95)).sum()) > int(((still_frames[0] > 0.05) & (still_frames[0] < 0.95)).sum())
