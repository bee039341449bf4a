"""The sampled camera (include/rtc.h rtc_sampling), the parts that need no GPU: a numpy / Python-float restatement of the rule, compared
with the library's own host evaluation (rtc_camera_rays without a scene: the function the generator kernel is compiled from), the
pinhole identity through the CPU emulator of the ray kernels, the draws, the validation rules through C and through `Sampling`, the
refusal of the libraries that have no such entry points, and the Rust mirror of the record."""
import ctypes as C
import math
import os

import numpy as np
import pytest

import foreign_flattener as ff
from raytracer_challenge_amd.cabi import load
from raytracer_challenge_amd import scenes
from raytracer_challenge_amd.backend import Backend, RtwError, SamplingC
from raytracer_challenge_amd.scene import Camera, Sampling, Vector
from test_area_lights_cpu import jitter as draw_of, splitmix64
from test_shim_layout import c_struct, rust_struct

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "raytracer_challenge_amd", "csrc", "librtc_amd.so")
M64 = (1 << 64) - 1
vp = C.c_void_p


# ---- the restatement of include/rtc.h rtc_sampling (shared with test_sampled_camera_gpu.py) ----------------------------------------
def sample_hash(seed: int, i: int, k: int) -> int:
    """h = m(m(m(seed) ^ i) ^ k)."""
    return splitmix64(splitmix64(splitmix64(seed & M64) ^ i) ^ k)


def subpixel(sp: Sampling, i: int, k: int):
    """(fx, fy) of sample k of pixel i."""
    n = sp.side
    sx, sy = k % n, k // n
    h = sample_hash(sp.seed, i, k)
    jx, jy = (draw_of(h, 0), draw_of(h, 1)) if sp.jitter else (0.5, 0.5)
    return (float(sx) + jx) / float(n), (float(sy) + jy) / float(n)


def sample_ray(rc: ff.RtcCameraC, sp: Sampling, i: int, k: int):
    """{o, d} of sample k of pixel i; every step one f64 operation (Python floats), left to right as the header states them."""
    m = list(rc.transform_inv)
    x, y = i % rc.hsize, i // rc.hsize
    fx, fy = subpixel(sp, i, k)
    xoffset = (float(x) + fx) * rc.pixel_size
    yoffset = (float(y) + fy) * rc.pixel_size
    world_x = rc.half_width - xoffset
    world_y = rc.half_height - yoffset

    def rows(px, py, pz):
        return [((m[4 * r] * px + m[4 * r + 1] * py) + m[4 * r + 2] * pz) + m[4 * r + 3] * 1.0 for r in range(3)]
    if sp.lens_radius > 0.0:
        h = sample_hash(sp.seed, i, k)
        R, F = sp.lens_radius, sp.focal_distance
        a, b = 2.0 * draw_of(h, 2) - 1.0, 2.0 * draw_of(h, 3) - 1.0
        if a == 0.0 and b == 0.0:
            lx = ly = 0.0
        else:
            if abs(a) > abs(b):
                r, phi = a, (math.pi / 4.0) * (b / a)
            else:
                r, phi = b, math.pi / 2.0 - (math.pi / 4.0) * (a / b)
            lx, ly = (R * r) * math.cos(phi), (R * r) * math.sin(phi)
        o = rows(lx, ly, 0.0)
        p = rows(world_x * F, world_y * F, -F)
    else:
        o = [m[3], m[7], m[11]]
        p = rows(world_x, world_y, -1.0)
    d = [p[0] - o[0], p[1] - o[1], p[2] - o[2]]
    mag = math.sqrt((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2])
    return o + [d[0] / mag, d[1] / mag, d[2] / mag]


def sample_rays(rc: ff.RtcCameraC, sp: Sampling, pixels) -> np.ndarray:
    return np.array([[sample_ray(rc, sp, int(i), k) for k in range(sp.samples)] for i in pixels], dtype=np.float64).reshape(len(pixels), sp.samples, 6)


def block_mean(frame: np.ndarray, hsize: int, vsize: int, side: int) -> np.ndarray:
    """The k-ordered mean (((c_0 + c_1) + ...) + c_{N-1}) / N of the side x side blocks of a (vsize*side, hsize*side) frame."""
    f = frame.reshape(vsize, side, hsize, side, 3)
    acc = f[:, 0, :, 0, :].copy()
    for k in range(1, side * side):
        acc = acc + f[:, k // side, :, k % side, :]
    return (acc / float(side * side)).reshape(-1, 3)


def samples_mean(colours: np.ndarray) -> np.ndarray:
    """The same over [n, N, 3] ray colours."""
    acc = colours[:, 0, :].copy()
    for k in range(1, colours.shape[1]):
        acc = acc + colours[:, k, :]
    return acc / float(colours.shape[1])


def rotated_camera():
    return Camera.new(9, 7, 1.1, Camera.transform(Vector.point(1.0, 2.0, -5.0), Vector.point(0.3, 0.5, 0.0), Vector.vector(0.1, 1.0, 0.2)))


def c_rays(lib, scene, rc, spc, n, idx=None, first=0):
    """rtc_camera_rays's status and rays for a raw SamplingC."""
    N = max(1, spc.side * spc.side) if spc.side <= 16 else 1
    out = np.full((n, N, 6), np.nan)
    idx_a = None if idx is None else np.ascontiguousarray(idx, dtype=np.uint64)
    code = lib.rtc_camera_rays(scene, C.byref(rc), C.byref(spc), None if idx is None else idx_a.ctypes.data, first, n, out.ctypes.data)
    return code, out


@pytest.fixture(scope="module")
def host():
    """librtc_amd.so without a device: loading it and the host-only entry points need none."""
    return Backend(LIB)


@pytest.fixture(scope="module")
def emu():
    from emu_lib import emu as load
    return load()


# ---- the rule ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("jit", [False, True])
@pytest.mark.parametrize("side", [1, 2, 3, 16])
def test_host_evaluation_is_the_restatement_bit_for_bit_without_a_lens(host, side, jit):
    cam = rotated_camera()
    rc = ff.make_camera(cam)
    sp = Sampling(side=side, jitter=jit, seed=0x1234567 + side)
    got = host.camera_rays(cam, sp)
    assert got.shape == (63, side * side, 6)
    # the library's own rtc_camera (rtw_make_camera) is the foreign flattener's, bit for bit: the restatement reads the latter
    want = sample_rays(rc, sp, range(63))
    assert np.array_equal(got.view(np.uint64), want.view(np.uint64))
    # a pixel list and a range give the listed pixels' rays
    idx = np.array([62, 0, 17, 17, 40], dtype=np.uint64)
    assert np.array_equal(host.camera_rays(cam, sp, pixel_indices=idx), got[idx.astype(np.int64)])
    code, part = c_rays(host.lib, None, rc, SamplingC.of(sp), 11, first=20)
    assert code == 0 and np.array_equal(part, got[20:31])


@pytest.mark.parametrize("jit", [False, True])
def test_host_evaluation_with_a_lens(host, jit):
    cam = rotated_camera()
    rc = ff.make_camera(cam)
    for side, R, F in ((1, 0.05, 1.0), (3, 0.2, 4.5), (4, 1.5, 0.3)):
        sp = Sampling(side=side, jitter=jit, seed=99, lens_radius=R, focal_distance=F)
        got, want = host.camera_rays(cam, sp), sample_rays(rc, sp, range(63))
        err = float(np.abs(got - want).max())
        assert err <= 1e-12, (side, R, F, err)   # only cos / sin may differ, by ulps
        # the origins lie on the lens disc and differ between the samples of a pixel; the directions are unit vectors
        T = np.array(cam.transform_matrix.m, dtype=np.float64)   # world -> camera space: the origins are (lx, ly, 0) there
        o_cam = got[..., :3] @ T[:3, :3].T + T[:3, 3]
        assert 0.0 < np.linalg.norm(o_cam[..., :2], axis=-1).max() <= R * (1.0 + 1e-9) and np.abs(o_cam[..., 2]).max() < 1e-9
        assert len({tuple(o) for o in got[5, :, :3]}) == side * side
        assert np.abs(np.linalg.norm(got[..., 3:], axis=-1) - 1.0).max() < 1e-15 * 4
    # the lens draws are hashed whether or not the positions are jittered: same origins either way
    a = host.camera_rays(cam, Sampling(side=2, jitter=False, seed=5, lens_radius=0.3, focal_distance=2.0))
    b = host.camera_rays(cam, Sampling(side=2, jitter=True, seed=5, lens_radius=0.3, focal_distance=2.0))
    assert np.array_equal(a[..., :3], b[..., :3]) and not np.array_equal(a[..., 3:], b[..., 3:])


def test_pinhole_identity_through_the_emulator(host, emu):
    """side = 1, no jitter, no lens: the rays are Camera::ray_at_pixel's -- the emulated kernels colour them exactly as they render the
    same pixels."""
    cam, world = scenes.chapter11_glass_air_bubble(24, 16)
    rays = host.camera_rays(cam, Sampling())
    assert rays.shape == (24 * 16, 1, 6)
    nw = emu.build_world(world)
    rgb_r, hits_r = emu.color_at(nw, rays.reshape(-1, 6), 5)
    rgb, hits = emu.render(nw, cam, 5)
    assert np.array_equal(rgb_r.view(np.uint64), rgb.view(np.uint64)) and hits_r.tobytes() == hits.tobytes()
    idx = np.array([5, 383, 100], dtype=np.uint64)
    rgb_l, _ = emu.color_at(nw, host.camera_rays(cam, Sampling(), pixel_indices=idx).reshape(-1, 6), 5)
    assert np.array_equal(rgb_l, rgb[idx.astype(np.int64)])


# ---- the draws ---------------------------------------------------------------------------------------------------------------------
def splitmix64_np(z: np.ndarray) -> np.ndarray:
    z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
    z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    return z ^ (z >> np.uint64(31))


def test_draws():
    seed = 0xC0FFEE
    i, k, j = np.meshgrid(np.arange(100, dtype=np.uint64), np.arange(250, dtype=np.uint64), np.arange(4, dtype=np.uint64), indexing="ij")
    h = splitmix64_np(splitmix64_np(splitmix64_np(np.full(i.shape, seed, dtype=np.uint64)) ^ i) ^ k)
    d = (splitmix64_np(h ^ j) >> np.uint64(11)).astype(np.float64) * 2.0 ** -53
    assert d.size == 100000
    for a, b, c in ((0, 0, 0), (99, 249, 3), (17, 100, 2)):   # the vectorised hash is the scalar one
        assert d[a, b, c] == draw_of(sample_hash(seed, a, b), c)
    assert d.min() >= 0.0 and d.max() < 1.0
    assert abs(float(d.mean()) - 0.5) <= 0.01   # standard error 0.0009: ten of them
    # stratified: each jittered sample inside its own cell
    for side in (2, 3, 16):
        sp = Sampling(side=side, jitter=True, seed=seed)
        for px in (0, 31, 62):
            for s in range(sp.samples):
                fx, fy = subpixel(sp, px, s)
                sx, sy = s % side, s // side
                assert sx / side <= fx < (sx + 1) / side and sy / side <= fy < (sy + 1) / side
    # and the grid: the cell centres
    assert [subpixel(Sampling(side=2), 7, s) for s in range(4)] == [(0.25, 0.25), (0.75, 0.25), (0.25, 0.75), (0.75, 0.75)]
    assert subpixel(Sampling(), 7, 0) == (0.5, 0.5)


def test_power_of_two_grid_is_a_finer_cameras_pixel_set():
    """What test_sampled_camera_gpu.py's oracle check rests on: for side 2 and 4 the unjittered offsets are, bit for bit, the pixel-centre
    offsets of a camera of side times the resolution and the same field of view (scaling by a power of two is exact); not for side 3."""
    differ = {2: 0, 3: 0, 4: 0}
    total = 0
    for fov in np.linspace(0.3, 2.4, 22):
        half_width = math.tan(fov / 2.0)
        for hsize in (37, 1920):
            for side in differ:
                ps, ps_fine = (half_width * 2.0) / float(hsize), (half_width * 2.0) / float(hsize * side)
                x, sx = np.meshgrid(np.arange(hsize, dtype=np.float64), np.arange(side, dtype=np.float64), indexing="ij")
                coarse = half_width - (x + (sx + 0.5) / float(side)) * ps
                fine = half_width - ((x * side + sx) + 0.5) * ps_fine
                differ[side] += int((coarse != fine).sum())
                total += coarse.size if side != 3 else 0
    assert total >= 250000 and differ[2] == 0 and differ[4] == 0 and differ[3] > 0, (total, differ)


def test_seeds(host):
    cam = rotated_camera()
    a = host.camera_rays(cam, Sampling(side=3, jitter=True, seed=1))
    b = host.camera_rays(cam, Sampling(side=3, jitter=True, seed=1))
    c = host.camera_rays(cam, Sampling(side=3, jitter=True, seed=2))
    assert np.array_equal(a, b) and not np.array_equal(a, c)
    # nothing but the pixel index and k enter: a pixel's rays do not depend on which pixels are asked for
    assert np.array_equal(host.camera_rays(cam, Sampling(side=3, jitter=True, seed=1), pixel_indices=np.array([44])), a[44:45])
    # without jitter and lens the seed is not read
    assert np.array_equal(host.camera_rays(cam, Sampling(side=3, seed=1)), host.camera_rays(cam, Sampling(side=3, seed=2)))


# ---- API and mirrors ---------------------------------------------------------------------------------------------------------------
def test_validation_through_c(host):
    lib = host.lib
    rc = ff.make_camera(rotated_camera())

    def code(side=1, flags=0, seed=0, R=0.0, F=1.0):
        return c_rays(lib, None, rc, SamplingC(side, flags, seed, R, F), 2)[0]
    assert code() == 0 and code(side=16, flags=1, R=0.5, F=3.0) == 0
    assert code(side=0) == 1                                        # RTC_ERR_INVALID
    assert code(flags=2) == 1 and code(flags=0x80000001) == 1
    assert code(R=-0.1) == 1 and code(R=math.inf) == 1 and code(R=math.nan) == 1
    assert code(R=0.1, F=0.0) == 1 and code(R=0.1, F=-1.0) == 1 and code(R=0.1, F=math.inf) == 1 and code(R=0.1, F=math.nan) == 1
    assert code(R=0.0, F=math.nan) == 0 and code(R=0.0, F=-1.0) == 0   # F is read only when R > 0
    assert code(side=17) == 2                                       # RTC_ERR_UNSUPPORTED
    assert b"side" in lib.rtc_last_error()
    spc = SamplingC(2, 0, 0, 0.0, 1.0)
    out = np.zeros((2, 4, 6))
    assert lib.rtc_camera_rays(None, None, C.byref(spc), None, 0, 2, out.ctypes.data) == 1     # NULL arguments
    assert lib.rtc_camera_rays(None, C.byref(rc), None, None, 0, 2, out.ctypes.data) == 1
    assert lib.rtc_camera_rays(None, C.byref(rc), C.byref(spc), None, 0, 2, None) == 1
    assert lib.rtc_camera_rays(None, C.byref(rc), C.byref(spc), None, 62, 2, out.ctypes.data) == 1   # range / index beyond the image
    assert c_rays(lib, None, rc, spc, 2, idx=[0, 63])[0] == 1
    assert lib.rtc_camera_rays(None, C.byref(rc), C.byref(spc), None, 0, 0, None) == 0
    # the render entry points validate before they touch a device
    for name, args in (("rtc_render_sampled", (None, C.byref(rc), C.byref(spc), 5, None, 0, 1, out.ctypes.data, None)),
                       ("rtc_render_sampled_rgb8", (None, C.byref(rc), C.byref(spc), 5, out.ctypes.data, None)),
                       ("rtc_render_sampled_bands_device", (None, C.byref(rc), C.byref(spc), 5, 8, 0, 1, 1, out.ctypes.data, None, 0, 1)),
                       ("rtc_render_multi_sampled", (None, C.byref(rc), C.byref(spc), 5, out.ctypes.data, None))):
        fn = getattr(lib, name)
        assert fn(*args) == 1, name   # NULL scene


def test_validation_through_sampling():
    s = Sampling()
    assert (s.side, s.jitter, s.seed, s.lens_radius, s.focal_distance, s.samples) == (1, False, 0, 0.0, 1.0, 1)
    assert Sampling(side=16, jitter=True, seed=M64, lens_radius=0.5, focal_distance=3.0).samples == 256
    Sampling(lens_radius=0.0, focal_distance=-1.0)   # F is read only when R > 0
    for bad in (dict(side=0), dict(side=17), dict(side=-1), dict(side=1.5), dict(lens_radius=-0.1), dict(lens_radius=math.inf), dict(lens_radius=math.nan),
                dict(lens_radius=0.1, focal_distance=0.0), dict(lens_radius=0.1, focal_distance=-2.0), dict(lens_radius=0.1, focal_distance=math.inf),
                dict(lens_radius=0.1, focal_distance=math.nan), dict(seed=-1), dict(seed=1 << 64)):
        with pytest.raises(ValueError):
            Sampling(**bad)
    with pytest.raises(Exception):
        s.side = 2   # frozen
    c = SamplingC.of(Sampling(side=3, jitter=True, seed=7, lens_radius=0.25, focal_distance=2.0))
    assert (c.side, c.flags, c.seed, c.lens_radius, c.focal_distance) == (3, 1, 7, 0.25, 2.0) and C.sizeof(SamplingC) == 32


def test_libraries_without_the_entry_points_refuse(emu, orc):
    cam, world = scenes.chapter11_glass_air_bubble(8, 8)
    for be in (emu, orc):
        nw = be.build_world(world)   # both still load and build worlds
        with pytest.raises(RtwError):
            be.render_sampled(nw, cam, Sampling(side=2))
        with pytest.raises(RtwError):
            be.camera_rays(cam, Sampling(side=2))
        assert be.render(nw, cam, 1)[0].shape == (64, 3)
    from raytracer_challenge_amd.image import Image
    with pytest.raises(RtwError):
        Image.par_render(cam, world, backend=emu, sampling=Sampling(side=2))
    assert Image.par_render(cam, world, fuel=1, backend=emu).pixels.shape == (64, 3)   # None takes today's route


def test_exports_and_rust_mirror():
    lib = load(LIB)
    for name in ("rtc_render_sampled", "rtc_render_sampled_rgb8", "rtc_render_sampled_bands_device", "rtc_render_multi_sampled", "rtc_camera_rays"):
        assert hasattr(lib, name), name
    h = open(os.path.join(ROOT, "include", "rtc.h")).read()
    rs = open(os.path.join(ROOT, "shim", "gpu.rs")).read()
    c, r = c_struct(h, "rtc_sampling"), rust_struct(rs, "RtcSampling")
    assert c == r == [("side", "u32", 0), ("flags", "u32", 0), ("seed", "u64", 0), ("lens_radius", "f64", 0), ("focal_distance", "f64", 0)]
    assert "RTC_SAMPLE_JITTER = 1u" in h and "pub const RTC_SAMPLE_JITTER: u32 = 1;" in rs
    assert "#define RTC_SAMPLES_MAX_SIDE 16" in h and "pub const RTC_SAMPLES_MAX_SIDE: u32 = 16;" in rs
    for name in ("rtc_render_sampled", "rtc_render_sampled_rgb8", "rtc_render_sampled_bands_device", "rtc_render_multi_sampled", "rtc_camera_rays"):
        assert "fn %s(" % name in rs, name
