"""The shutter (include/rtc.h rtc_shutter), the parts that need no GPU: a Python-int restatement of the dealing rule, compared with the
library's own host evaluation (rtc_shutter_deal without a scene: the function the dealing kernels are compiled from), the clamp of the
hashed draw, the sequential split, every limit through C, the argument errors of `Shutter` / `Image.par_render_shutter`, and the mirrors
of the record."""
import ctypes as C
import math
import os

import numpy as np
import pytest

import foreign_flattener as ff
from raytracer_challenge_amd.cabi import load
from raytracer_challenge_amd import scenes
from raytracer_challenge_amd.backend import Backend, RtwError, SamplingC, ShutterC
from raytracer_challenge_amd.image import Image
from raytracer_challenge_amd.scene import Camera, Matrix, Sampling, Shutter
from test_area_lights_cpu import jitter as draw_of
from test_sampled_camera_cpu import sample_hash, splitmix64_np
from test_shim_layout import c_struct, rust_struct

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "raytracer_challenge_amd", "csrc", "librtc_amd.so")
vp = C.c_void_p
OK, INVALID, UNSUPPORTED = 0, 1, 2

FRAME = (37, 19)
LIST7 = np.array([702, 0, 36, 37, 350, 350, 1], dtype=np.uint64)   # 7 pixels of the 37x19 frame, one of them twice


# ---- the restatement of include/rtc.h rtc_shutter (shared with test_shutter_gpu.py) -------------------------------------------------
def draw_pose(u: float, K: int) -> int:
    """s = (uint32_t)(u * (double)K), held to K - 1."""
    return min(int(u * float(K)), K - 1)


_draws = {}


def time_draws(sp: Sampling, pixels) -> list:
    """u = rtc_area_jitter(h, 4) of every (pixel, k), pixel-major; SplitMix64 in Python ints.  Kept per (seed, side, pixels): K does not enter."""
    key = (sp.seed, sp.side, tuple(int(i) for i in pixels))
    if key not in _draws:
        _draws[key] = [draw_of(sample_hash(sp.seed, i, k), 4) for i in key[2] for k in range(sp.samples)]
    return _draws[key]


def poses_of(sp: Sampling, hashed: bool, K: int, pixels) -> np.ndarray:
    """Pose of every sample id (slot * N + k) of the listed pixels."""
    N = sp.samples
    if hashed:
        return np.array([draw_pose(u, K) for u in time_draws(sp, pixels)], dtype=np.int64)
    return np.array([(k * K) // N for _ in pixels for k in range(N)], dtype=np.int64)


def poses_np(sp: Sampling, hashed: bool, K: int, pixels) -> np.ndarray:
    """poses_of on numpy uint64 arrays (products wrap modulo 2^64 as the C ones do), for millions of samples; restated from include/rtc.h
    like the scalar one:  sequential s = (k * K) / N;  hashed h = m(m(m(seed) ^ i) ^ k), u = (m(h ^ 4) >> 11) * 2^-53 (rtc_area_jitter(h, 4):
    53 bits, exact in a double), t = u * (double)K, s = (uint32_t)t held to K - 1."""
    pixels = np.ascontiguousarray(pixels, dtype=np.uint64).reshape(-1)
    N = sp.samples
    k = np.arange(N, dtype=np.uint64)
    if not hashed:
        return np.tile(((k * np.uint64(K)) // np.uint64(N)).astype(np.int64), pixels.size)
    seed = splitmix64_np(np.array([sp.seed & 0xFFFFFFFFFFFFFFFF], dtype=np.uint64))
    h = splitmix64_np(splitmix64_np(seed ^ pixels)[:, None] ^ k[None, :])
    u = (splitmix64_np(h ^ np.uint64(4)) >> np.uint64(11)).astype(np.float64) * 2.0 ** -53
    s = (u * float(K)).astype(np.int64)         # t >= 0: the conversion truncates, as the cast does
    return np.minimum(s, K - 1).reshape(-1)


def deal(poses: np.ndarray, K: int):
    """(order, offsets): the ids pose-major and ascending within a pose -- a stable sort by pose --, and where each pose's run starts."""
    order = np.argsort(poses, kind="stable").astype(np.uint32)
    offsets = np.concatenate(([0], np.cumsum(np.bincount(poses, minlength=K)))).astype(np.uint64)
    return order, offsets


@pytest.fixture(scope="module")
def host():
    """librtc_amd.so without a device: loading it and the host-only entry points need none."""
    return Backend(LIB)


# ---- the rule ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hashed", [False, True])
@pytest.mark.parametrize("side", [1, 3, 4, 16])
def test_host_dealing_is_the_restatement(host, side, hashed):
    frame_pixels = list(range(FRAME[0] * FRAME[1]))
    for seed in (0, 0x9E3779B97F4A7C15):
        sp = Sampling(side=side, seed=seed)
        N = sp.samples
        for K in (1, 2, 3, 5, 64):
            for pixels, kw in ((frame_pixels, dict(n=len(frame_pixels))), ([int(i) for i in LIST7], dict(pixel_indices=LIST7))):
                if not hashed and K > N:   # some poses would never be sampled
                    with pytest.raises(RtwError):
                        host.shutter_deal(FRAME[0], K, sp, Shutter(hashed), **kw)
                    continue
                order, offsets = host.shutter_deal(FRAME[0], K, sp, Shutter(hashed), **kw)
                want_order, want_offsets = deal(poses_of(sp, hashed, K, pixels), K)
                m = len(pixels) * N
                assert offsets.shape == (K + 1,) and offsets[0] == 0 and offsets[K] == m and (np.diff(offsets.astype(np.int64)) >= 0).all()
                assert np.array_equal(np.sort(order), np.arange(m, dtype=np.uint32))          # a permutation
                assert np.array_equal(offsets, want_offsets), (side, hashed, seed, K)
                assert np.array_equal(order, want_order), (side, hashed, seed, K)
    # a range that is not whole rows deals like the same pixels listed; nothing but the pixel index and k enter
    sp = Sampling(side=3, seed=11)
    a = host.shutter_deal(FRAME[0], 5, sp, Shutter(hashed), first=40, n=50)
    b = host.shutter_deal(FRAME[0], 5, sp, Shutter(hashed), pixel_indices=np.arange(40, 90, dtype=np.uint64))
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


@pytest.mark.parametrize("hashed", [False, True])
def test_the_vectorised_restatement_is_the_scalar_one(hashed):
    """poses_np against the Python-int poses_of: the whole 37x19 frame and LIST7, K in {1, 3, 5, 64}."""
    frame_pixels = list(range(FRAME[0] * FRAME[1]))
    for sp in (Sampling(side=3, seed=0), Sampling(side=4, seed=0x9E3779B97F4A7C15), Sampling(side=16, seed=1234), Sampling(side=1, seed=7)):
        for K in (1, 3, 5, 64):
            for pixels in (frame_pixels, [int(i) for i in LIST7]):
                want = poses_of(sp, hashed, K, pixels)
                got = poses_np(sp, hashed, K, pixels)
                assert got.dtype == np.int64 and got.shape == want.shape and np.array_equal(got, want), (sp, hashed, K, len(pixels))
                if hashed and K > 1 and len(pixels) > 7:
                    assert got.min() == 0 and got.max() == K - 1
    # indices past 2^32 hash as 64-bit words
    far = [(1 << 33) + 5, (1 << 38) - 1]
    assert np.array_equal(poses_np(Sampling(side=3, seed=5), True, 7, far), poses_of(Sampling(side=3, seed=5), True, 7, far))


# 2^22 samples are one default chunk of a real frame (16 384 blocks of 256); the device's count table has K entries per block
BIG_DEALS = [  # (hsize, vsize, side, K, hashed)
    (512, 512, 4, 5, True),        # 81 920 entries: three scan levels on the device
    (128, 129, 4, 64, True),       # 264 192 samples, 1 032 blocks: 66 048 entries -> 258 -> 2
    (512, 512, 4, 16, False),      # 262 144 entries; every wave of 64 samples holds each pose four times
]


def big_deal_case(hsize, vsize, side, K, hashed, pixels=None):
    """(sampling, shutter, the restated dealing) of a large case; the seed follows the shape."""
    sp, sh = Sampling(side=side, seed=1000 * K + hsize + vsize), Shutter(hashed)
    px = np.arange(hsize * vsize, dtype=np.uint64) if pixels is None else pixels
    poses = poses_np(sp, hashed, K, px)
    return sp, sh, poses, deal(poses, K)


def check_dealing_properties(order, offsets, poses, K):
    """What holds without any reference dealing: a permutation, ascending inside every run, offsets = prefix sums of the poses' counts."""
    m = poses.size
    seen = np.zeros(m, dtype=bool)
    assert order.shape == (m,) and int(order.max()) < m
    seen[order] = True
    assert seen.all()
    assert np.array_equal(offsets, np.concatenate(([0], np.cumsum(np.bincount(poses, minlength=K)))).astype(np.uint64))
    rising = np.diff(order.astype(np.int64)) > 0
    rising[offsets[1:K].astype(np.int64)[(offsets[1:K] > 0) & (offsets[1:K] < m)] - 1] = True    # (a run's first id may be below the last of the run before)
    assert rising.all()
    assert np.array_equal(poses[order], np.repeat(np.arange(K), np.diff(offsets.astype(np.int64))))


@pytest.mark.parametrize("hsize,vsize,side,K,hashed", BIG_DEALS)
def test_host_dealing_of_a_production_chunk_is_the_restatement(host, hsize, vsize, side, K, hashed):
    sp, sh, poses, (want_order, want_offsets) = big_deal_case(hsize, vsize, side, K, hashed)
    order, offsets = host.shutter_deal(hsize, K, sp, sh, n=hsize * vsize)
    assert np.array_equal(offsets, want_offsets), (offsets, want_offsets)
    assert np.array_equal(order, want_order)
    check_dealing_properties(order, offsets, poses, K)


def test_hashed_poses_depend_on_the_seed_and_not_on_jitter(host):
    a = host.shutter_deal(FRAME[0], 5, Sampling(side=3, seed=1), Shutter(), n=703)
    b = host.shutter_deal(FRAME[0], 5, Sampling(side=3, seed=2), Shutter(), n=703)
    c = host.shutter_deal(FRAME[0], 5, Sampling(side=3, seed=1, jitter=True, lens_radius=0.2, focal_distance=3.0), Shutter(), n=703)
    assert not np.array_equal(a[0], b[0]) and np.array_equal(a[0], c[0]) and np.array_equal(a[1], c[1])
    # every pose gets about a fifth: 6 327 draws, binomial sigma = sqrt(6327 * 0.2 * 0.8) = 31.8; 6 sigma
    assert (np.abs(np.diff(a[1].astype(np.int64)) - 6327 / 5.0) <= 6.0 * math.sqrt(6327 * 0.2 * 0.8)).all()


def test_the_clamp(host):
    u = 1.0 - 2.0 ** -53   # the largest draw
    for K in (3, 7, 64):
        assert draw_pose(u, K) <= K - 1
        assert host.lib.rtc_shutter_draw_pose(u, K) == draw_pose(u, K) <= K - 1
        assert host.lib.rtc_shutter_draw_pose(0.0, K) == 0
        assert host.lib.rtc_shutter_draw_pose(1.0, K) == K - 1     # not a draw: what the clamp is for
    assert [host.lib.rtc_shutter_draw_pose(p / 3.0 + 1e-9, 3) for p in range(3)] == [0, 1, 2]


@pytest.mark.parametrize("side,K", [(1, 1), (3, 2), (3, 9), (4, 3), (4, 5), (4, 16), (16, 64), (16, 5)])
def test_sequential_mode_splits_every_pixel_evenly(host, side, K):
    sp = Sampling(side=side, seed=3)
    N = sp.samples
    order, offsets = host.shutter_deal(FRAME[0], K, sp, Shutter(hashed=False), pixel_indices=LIST7)
    for p in range(K):
        run = order[int(offsets[p]):int(offsets[p + 1])].astype(np.int64)
        per_pixel = np.bincount(run // N, minlength=len(LIST7))
        assert ((per_pixel == N // K) | (per_pixel == -(-N // K))).all(), (side, K, p, per_pixel)
        assert (np.diff(run) > 0).all()                    # ascending within the pose
        k = run % N
        assert ((k * K) // N == p).all()


# ---- limits ------------------------------------------------------------------------------------------------------------------------
def test_every_limit_through_c_without_a_device(host):
    lib = host.lib
    order, offsets = np.zeros(7 * 256, dtype=np.uint32), np.zeros(66, dtype=np.uint64)

    def deal_code(K=3, flags=1, sh=True, sp=True, side=3, sflags=0, R=0.0, F=1.0, hsize=37, n=7, order_p=order.ctypes.data, offsets_p=offsets.ctypes.data):
        shc, spc = ShutterC(flags, 0), SamplingC(side, sflags, 0, R, F)
        return lib.rtc_shutter_deal(None, hsize, K, C.byref(shc) if sh else None, C.byref(spc) if sp else None, LIST7.ctypes.data, 0, n, order_p, offsets_p)
    assert deal_code() == OK and deal_code(flags=0) == OK and deal_code(K=64) == OK and deal_code(K=9, flags=0) == OK
    assert deal_code(K=0) == INVALID and b"n_poses" in lib.rtc_last_error()
    assert deal_code(sh=False) == INVALID and deal_code(sp=False) == INVALID
    assert deal_code(flags=2) == INVALID and deal_code(flags=0x80000001) == INVALID and b"flag" in lib.rtc_last_error()
    assert deal_code(K=10, flags=0) == INVALID and b"more poses than samples" in lib.rtc_last_error()       # K > N, sequential
    assert deal_code(K=2, flags=0, side=1) == INVALID and deal_code(K=2, flags=1, side=1) == OK
    assert deal_code(K=65) == UNSUPPORTED and deal_code(K=65, flags=0, side=16) == UNSUPPORTED and b"RTC_SHUTTER_MAX_POSES" in lib.rtc_last_error()
    # everything check_sampling refuses
    assert deal_code(side=0) == INVALID and deal_code(sflags=2) == INVALID and deal_code(R=-0.1) == INVALID and deal_code(R=math.nan) == INVALID
    assert deal_code(R=0.1, F=0.0) == INVALID and deal_code(R=0.1, F=math.inf) == INVALID and deal_code(side=17) == UNSUPPORTED
    # the dealing's own arguments
    assert deal_code(order_p=None) == INVALID and deal_code(offsets_p=None) == INVALID and deal_code(hsize=0) == INVALID
    assert deal_code(n=0, order_p=None) == OK and not offsets[:4].any()

    # the render entry points: the shutter's own numbers before anything else, then the arrays; no device is touched
    cam = Camera.new(37, 19, 1.0, Matrix.id())
    cams = (ff.RtcCameraC * 3)(*[ff.make_camera(cam)] * 3)
    scenes_null = (vp * 3)()      # three NULL entries
    rgb = np.zeros((7, 3))
    rgb8 = np.zeros(703 * 3, dtype=np.uint8)

    def render_code(K=3, flags=1, sh=True, side=3, scenes_p=scenes_null, cams_p=cams, out=rgb.ctypes.data):
        shc, spc = ShutterC(flags, 0), SamplingC(side, 0, 0, 0.0, 1.0)
        a = lib.rtc_render_shutter(scenes_p, cams_p, K, C.byref(shc) if sh else None, C.byref(spc), 5, LIST7.ctypes.data, 0, 7, out, None)
        err = lib.rtc_last_error()
        b = lib.rtc_render_shutter_rgb8(scenes_p, cams_p, K, C.byref(shc) if sh else None, C.byref(spc), 5, rgb8.ctypes.data, None)
        assert a == b, (a, b)
        return a, err
    assert render_code(K=0)[0] == INVALID and render_code(sh=False)[0] == INVALID and render_code(flags=4)[0] == INVALID
    assert render_code(K=65, scenes_p=None, cams_p=None)[0] == UNSUPPORTED         # before the NULL arrays are looked at
    assert render_code(K=3, flags=0, side=1, scenes_p=None)[0] == INVALID and b"more poses" in lib.rtc_last_error()
    assert render_code(side=0)[0] == INVALID and render_code(side=17, scenes_p=None)[0] == UNSUPPORTED
    code, err = render_code(scenes_p=None)
    assert code == INVALID and b"NULL argument" in err
    code, err = render_code(cams_p=None)
    assert code == INVALID and b"NULL argument" in err
    code, err = render_code()
    assert code == INVALID and b"NULL scene" in err                                # NULL entries
    odd = (ff.RtcCameraC * 3)(ff.make_camera(cam), ff.make_camera(Camera.new(37, 20, 1.0, Matrix.id())), ff.make_camera(cam))
    code, err = render_code(cams_p=odd)
    assert code == INVALID and b"hsize or vsize differ" in err
    odd = (ff.RtcCameraC * 3)(ff.make_camera(cam), ff.make_camera(cam), ff.make_camera(Camera.new(36, 19, 1.0, Matrix.id())))
    code, err = render_code(cams_p=odd)
    assert code == INVALID and b"hsize or vsize differ" in err
    assert lib.rtc_render_shutter_rgb8(scenes_null, cams, 3, C.byref(ShutterC(1, 0)), C.byref(SamplingC(3, 0, 0, 0.0, 1.0)), 5, None, None) == INVALID


# ---- the Python layer ---------------------------------------------------------------------------------------------------------------
def test_shutter_and_par_render_shutter_argument_errors(host):
    assert Shutter().hashed is True and Shutter(hashed=False).hashed is False
    for bad in (1, 0, None, "yes"):
        with pytest.raises(ValueError):
            Shutter(hashed=bad)
    with pytest.raises(Exception):
        Shutter().hashed = False   # frozen
    assert (ShutterC.of(Shutter()).flags, ShutterC.of(Shutter(hashed=False)).flags) == (1, 0)
    poses = scenes.motion_showcase(8, 8, 3)
    assert len(poses) == 3 and all(isinstance(c, Camera) and (c.hsize, c.vsize) == (8, 8) for c, _ in poses)
    assert poses[0][1] is not poses[1][1] and poses[0][0].transform_matrix.flat() != poses[2][0].transform_matrix.flat()
    with pytest.raises(ValueError):
        scenes.motion_showcase(8, 8, 0)
    sp = Sampling(side=2)
    for bad_poses in ([], [poses[0][0]], [(poses[0][1], poses[0][0])], [poses[0], (Camera.new(9, 8, 1.0, Matrix.id()), poses[1][1])]):
        with pytest.raises(ValueError):
            Image.par_render_shutter(bad_poses, sp, backend=host)
    with pytest.raises(ValueError):
        Image.par_render_shutter(poses, None, backend=host)
    with pytest.raises(ValueError):
        Image.par_render_shutter(poses, sp, shutter=True, backend=host)
    with pytest.raises(ValueError):
        Image.par_render_shutter(scenes.motion_showcase(8, 8, 5), sp, shutter=Shutter(hashed=False), backend=host)   # K = 5 > N = 4
    with pytest.raises(ValueError):
        host.render_shutter([], [], sp, Shutter())
    with pytest.raises(ValueError):
        host.shutter_deal(37, 3, sp, Shutter())   # neither a list nor a count


def test_libraries_without_the_entry_points_refuse(orc):
    poses = scenes.motion_showcase(8, 8, 2)
    with pytest.raises(RtwError):
        orc.shutter_deal(8, 2, Sampling(side=2), Shutter(), n=4)
    with pytest.raises(RtwError):
        Image.par_render_shutter(poses, Sampling(side=2), backend=orc)


def test_exports_and_mirrors():
    lib = load(LIB)
    names = ("rtc_render_shutter", "rtc_render_shutter_rgb8", "rtc_shutter_deal")
    for name in names + ("rtc_shutter_draw_pose",):
        assert hasattr(lib, name), name
    h = open(os.path.join(ROOT, "include", "rtc.h")).read()
    rs = open(os.path.join(ROOT, "shim", "gpu.rs")).read()
    c, r = c_struct(h, "rtc_shutter"), rust_struct(rs, "RtcShutter")
    assert c == r == [("flags", "u32", 0), ("_pad", "u32", 0)]
    assert C.sizeof(ShutterC) == 4 * len(c) == 8 and [f[0] for f in ShutterC._fields_] == [f[0] for f in c]
    assert "RTC_SHUTTER_HASHED = 1u" in h and "pub const RTC_SHUTTER_HASHED: u32 = 1;" in rs
    assert "#define RTC_SHUTTER_MAX_POSES 64" in h and "pub const RTC_SHUTTER_MAX_POSES: u32 = 64;" in rs
    for name in ("rtc_render_shutter", "rtc_render_shutter_rgb8"):
        assert "fn %s(" % name in rs, name
    from raytracer_challenge_amd.scene import SHUTTER_MAX_POSES
    assert SHUTTER_MAX_POSES == 64
