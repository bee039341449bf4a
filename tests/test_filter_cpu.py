"""Pixel reconstruction filters (include/rtc.h rtc_filter), the parts that need no GPU: a Python-float restatement of the rule, looped in
the defined order, compared with the library's own host evaluation (rtc_filter_frame without a scene: the function the gather kernel is
compiled from); the box identity, normalisation, the zero-weight rule, the validation rules through C and through `Filter`, the refusal
of the libraries that have no such entry points, and the Rust mirror of the record."""
import ctypes as C
import math
import os

import numpy as np
import pytest

import foreign_flattener as ff
from raytracer_challenge_amd.cabi import load
from raytracer_challenge_amd import scenes
from raytracer_challenge_amd.backend import Backend, FilterC, RtwError, SamplingC
from raytracer_challenge_amd.image import Image
from raytracer_challenge_amd.scene import FILTER_KINDS, Adaptive, Filter, Sampling
from test_sampled_camera_cpu import samples_mean, subpixel
from test_shim_layout import c_struct, rust_struct

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "raytracer_challenge_amd", "csrc", "librtc_amd.so")
vp = C.c_void_p

FRAMES = [(1, 1), (1, 7), (7, 1), (9, 5), (13, 11)]   # (hsize, vsize); 9x5: the radius-3 window is taller than the image
RADII = [0.5, 1.0, 1.5, 2.0, 3.0]


def filters(radius):
    return [Filter.box(radius), Filter.tent(radius), Filter.gaussian(radius, 2.0), Filter.mitchell(radius)]


# ---- the restatement of include/rtc.h rtc_filter (shared with test_filter_gpu.py) --------------------------------------------------
def window(radius: float) -> int:
    return int(math.ceil(radius - 0.5))


def f_of(flt: Filter, d: float) -> float:
    a, r = abs(d), flt.radius
    if not a < r:
        return 0.0
    if flt.kind == "box":
        return 1.0
    if flt.kind == "tent":
        return 1.0 - a / r
    if flt.kind == "gaussian":
        return math.exp(-flt.alpha * a * a) - math.exp(-flt.alpha * r * r)
    t = (a + a) / r
    if t < 1.0:
        return ((((7.0 * t - 12.0) * t) * t) + 16.0 / 3.0) / 6.0
    return ((((-7.0 / 3.0) * t + 12.0) * t - 20.0) * t + 32.0 / 3.0) / 6.0


_offsets = {}


def offsets_of(hsize: int, vsize: int, sp: Sampling):
    """(fx, fy) of every sample of the frame: [pixel][k], once per frame and sampling."""
    key = (hsize, vsize, sp)
    if key not in _offsets:
        _offsets[key] = [[subpixel(sp, i, k) for k in range(sp.samples)] for i in range(hsize * vsize)]
    return _offsets[key]


def filter_frame_py(hsize: int, vsize: int, sp: Sampling, flt: Filter, samples: np.ndarray, off=None) -> np.ndarray:
    """The rule over `samples` ([hsize*vsize, N, 3]); every step one f64 operation (Python floats), in the order the header states.
    off: the samples' positions [pixel][k] = (fx, fy) where they are not to be `subpixel`'s."""
    W, N = window(flt.radius), sp.samples
    off = offsets_of(hsize, vsize, sp) if off is None else off
    col = samples.reshape(hsize * vsize, N, 3).tolist()
    out = np.empty((hsize * vsize, 3))
    for y in range(vsize):
        for x in range(hsize):
            num, den = [0.0, 0.0, 0.0], 0.0
            for qy in range(max(0, y - W), min(vsize - 1, y + W) + 1):
                for qx in range(max(0, x - W), min(hsize - 1, x + W) + 1):
                    q = qy * hsize + qx
                    for k in range(N):
                        fx, fy = off[q][k]
                        dx = float(qx - x) + (fx - 0.5)
                        dy = float(qy - y) + (fy - 0.5)
                        w = f_of(flt, dx) * f_of(flt, dy)
                        if w == 0.0:
                            continue
                        c = col[q][k]
                        num = [num[0] + w * c[0], num[1] + w * c[1], num[2] + w * c[2]]
                        den = den + w
            out[y * hsize + x] = [n / den if den != 0.0 else (math.nan if n == 0.0 or n != n else math.copysign(math.inf, n)) for n in num]
    return out


def random_samples(hsize, vsize, N, seed, wild=False):
    """Seeded colours in [0, 1); wild: some negative, some > 1, a handful NaN or +-inf."""
    rng = np.random.default_rng(seed)
    s = rng.random((hsize * vsize, N, 3))
    if wild:
        s = s * 3.0 - 1.0
        flat = s.reshape(-1)
        for j, v in zip(rng.choice(flat.size, size=min(6, flat.size), replace=False), (np.nan, np.inf, -np.inf, np.nan, np.inf, -np.inf)):
            flat[j] = v
    return s


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def same_bits(a, b):
    """Bit-equal, any NaN counting as equal to any NaN (payloads are not part of the rule)."""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    nan = np.isnan(a) & np.isnan(b)
    return a.shape == b.shape and bool(np.all(nan | (bits(a) == bits(b))))


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
@pytest.mark.parametrize("side", [1, 2, 3])
def test_host_evaluation_is_the_restatement(host, side, jit):
    worst = 0.0
    for hsize, vsize in FRAMES:
        sp = Sampling(side=side, jitter=jit, seed=0xF117 + side)
        samples = random_samples(hsize, vsize, sp.samples, 1000 * hsize + 10 * vsize + side)
        for radius in RADII:
            for flt in filters(radius):
                got = host.filter_frame(samples, hsize, vsize, sp, flt)
                want = filter_frame_py(hsize, vsize, sp, flt, samples)
                assert got.shape == (hsize * vsize, 3)
                if flt.kind == "gaussian":   # exp: the C library's against Python's (the same libm here, but not by contract)
                    err = float(np.abs(got - want).max())
                    worst = max(worst, err)
                    assert err <= 1e-12, ((hsize, vsize), side, jit, flt, err)
                else:
                    assert np.array_equal(bits(got), bits(want)), ((hsize, vsize), side, jit, flt)
    print("side %d jitter %s: max |host - restatement| over the Gaussian cases = %.3e" % (side, jit, worst))


def test_the_filters_positions_are_the_rays_positions(host):
    """filter_weights.h restates rtc_sample_ray's sub-pixel position (factoring it out changed the generator kernel's code).  The two are
    pinned against each other: through a camera with the identity transform, half_width = half_height = 0 and pixel_size = 2^-6 a pinhole ray
    of rtc_camera_rays is normalise(-(x + fx) / 64, -(y + fy) / 64, -1) with exact products, so fx = -64 * (d_x / -d_z) - x up to the roundings of
    the normalisation, the quotient and x + fx: a few ulp of 8, under 1e-14.  The restated rule fed with THOSE positions must give
    rtc_filter_frame's frame; a tent's weight moves by at most |dfx| / r, so 1e-12 covers it, while a position from another hash, draw
    or cell is off by about the width of a cell and moves a pixel of these random colours by about 1e-1."""
    from test_sampled_camera_cpu import c_rays
    lib = host.lib
    hsize, vsize = 8, 4
    rc = ff.RtcCameraC()
    rc.hsize, rc.vsize, rc.half_width, rc.half_height, rc.pixel_size = hsize, vsize, 0.0, 0.0, 2.0 ** -6
    for j in range(16):
        rc.transform_inv[j] = 1.0 if j % 5 == 0 else 0.0
    for side, jit in ((1, True), (3, True), (4, False), (2, True)):
        sp = Sampling(side=side, jitter=jit, seed=0xABCD + side)
        code, rays = c_rays(lib, None, rc, SamplingC.of(sp), hsize * vsize)
        assert code == 0 and np.array_equal(rays[..., :3], np.zeros_like(rays[..., :3]))
        px = np.arange(hsize * vsize)
        fx = -64.0 * (rays[..., 3] / -rays[..., 5]) - (px % hsize)[:, None]
        fy = -64.0 * (rays[..., 4] / -rays[..., 5]) - (px // hsize)[:, None]
        assert fx.min() >= -1e-14 and fx.max() < 1.0 + 1e-14 and fy.min() >= -1e-14 and fy.max() < 1.0 + 1e-14
        own = np.array(offsets_of(hsize, vsize, sp))
        assert float(np.abs(own[..., 0] - fx).max()) <= 1e-14 and float(np.abs(own[..., 1] - fy).max()) <= 1e-14
        off = [[(float(fx[i, k]), float(fy[i, k])) for k in range(sp.samples)] for i in range(hsize * vsize)]
        samples = random_samples(hsize, vsize, sp.samples, 11 + side)
        for flt in (Filter.tent(1.5), Filter.tent(0.75), Filter.mitchell(2.0)):
            got = host.filter_frame(samples, hsize, vsize, sp, flt)
            err = float(np.abs(got - filter_frame_py(hsize, vsize, sp, flt, samples, off)).max())
            assert err <= 1e-12, (side, jit, flt, err)
        # the pin can fail: the positions of another seed are another frame
        other = Sampling(side=side, jitter=True, seed=1)
        assert float(np.abs(host.filter_frame(samples, hsize, vsize, other, Filter.tent(1.5)) - filter_frame_py(hsize, vsize, sp, Filter.tent(1.5), samples, off)).max()) > 1e-3 or not jit


@pytest.mark.parametrize("jit", [False, True])
def test_box_of_half_a_pixel_is_the_sample_mean(host, jit):
    for hsize, vsize in FRAMES:
        for side in (1, 2, 3, 16):
            sp = Sampling(side=side, jitter=jit, seed=5)
            samples = random_samples(hsize, vsize, sp.samples, 77 + side, wild=True)
            got = host.filter_frame(samples, hsize, vsize, sp, Filter.box(0.5))
            assert same_bits(got, samples_mean(samples)), ((hsize, vsize), side, jit)


def weights_py(hsize: int, vsize: int, sp: Sampling, flt: Filter):
    """Per output pixel, the non-zero weights of the rule in its order."""
    W, off, out = window(flt.radius), offsets_of(hsize, vsize, sp), []
    for y in range(vsize):
        for x in range(hsize):
            ws = []
            for qy in range(max(0, y - W), min(vsize - 1, y + W) + 1):
                for qx in range(max(0, x - W), min(hsize - 1, x + W) + 1):
                    for fx, fy in off[qy * hsize + qx]:
                        w = f_of(flt, float(qx - x) + (fx - 0.5)) * f_of(flt, float(qy - y) + (fy - 0.5))
                        if w != 0.0:
                            ws.append(w)
            out.append(ws)
    return out


def test_a_constant_colour_comes_back(host):
    """Normalisation, Mitchell's negative lobes included.  With n samples of non-zero weight, u = 2^-53 and S = sum |w| / |sum w| (1 for
    the non-negative kinds), the sums in the rule's order satisfy |num - c sum w| <= n u |c| sum |w| and |den - sum w| <= (n - 1) u sum |w|
    to first order (one product and n - 1 additions per term), the quotient adds u, and ulp(c) >= u |c|: the pixel is within
    (2 n - 1) S + 1 ulp of c, asserted per pixel with 1 % for the higher-order terms.  That is at most the issue's 4 ulp exactly where a
    pixel has ONE weighted sample (radius 0.5 with one sample per pixel; an unjittered centre sample with radius 1.0, whose neighbours sit
    at a == r), and there 4 ulp are asserted for every kind.  Beyond it the rule's own arithmetic exceeds 4 ulp -- measured on
    the host function over c = 0.3, 1.7, -0.1 on a 9x5 frame, worst pixel: box 3.0 over 3x3 samples (n = 225 equal terms, whose roundings
    do not cancel) 34 ulp; tent 15; Gaussian 15; Mitchell 20, and 592 for Mitchell 1.0 over one jittered sample per pixel, where the negative
    lobes leave S near 150 -- so no flat figure is asserted there."""
    worst_small, worst_ratio = 0.0, 0.0
    for side in (1, 2, 3):
        for jit in (False, True):
            sp = Sampling(side=side, jitter=jit, seed=31)
            for radius in RADII:
                for flt in filters(radius):
                    ws = weights_py(9, 5, sp, flt)
                    bound = np.array([((2 * len(w) - 1) * (sum(abs(v) for v in w) / abs(sum(w))) + 1.0) * 1.01 for w in ws])
                    single = all(len(w) == 1 for w in ws)
                    assert single == ((side == 1 and radius == 0.5) or (side == 1 and not jit and radius == 1.0)), (side, jit, flt)
                    for c in (0.3, 1.7, -0.1):
                        got = host.filter_frame(np.full((45, sp.samples, 3), c), 9, 5, sp, flt)
                        u = np.abs(got - c).max(axis=1) / np.spacing(abs(c))
                        assert (u <= bound).all(), (c, side, jit, flt, float((u / bound).max()))
                        worst_ratio = max(worst_ratio, float((u / bound).max()))
                        if single:
                            worst_small = max(worst_small, float(u.max()))
                            assert u.max() <= 4.0, (c, side, jit, flt, float(u.max()))
    print("constant colour: worst error of the one-sample supports = %.1f ulp; worst error / bound over every case = %.3f" % (worst_small, worst_ratio))


def test_zero_weights(host):
    sp = Sampling()   # one centre sample: the neighbours of a radius-1 box sit at a == r exactly
    samples = random_samples(9, 5, 1, 3, wild=True)
    got = host.filter_frame(samples, 9, 5, sp, Filter.box(1.0))
    assert same_bits(got, samples[:, 0, :])
    # a NaN sample changes only its own pixel
    clean = random_samples(9, 5, 1, 4)
    dirty = clean.copy()
    dirty[2 * 9 + 4, 0, 1] = np.nan
    a, b = host.filter_frame(clean, 9, 5, sp, Filter.box(1.0)), host.filter_frame(dirty, 9, 5, sp, Filter.box(1.0))
    changed = np.flatnonzero((bits(a) != bits(b)).any(axis=1))
    assert changed.tolist() == [2 * 9 + 4] and np.isnan(b[2 * 9 + 4, 1]) and np.isfinite(b[2 * 9 + 4, [0, 2]]).all()
    # a tent of radius 1.5 reaches the 3x3 neighbourhood and nothing else
    dirty[2 * 9 + 4, 0, :] = np.nan
    t = host.filter_frame(dirty, 9, 5, sp, Filter.tent(1.5))
    want = {y * 9 + x for y in (1, 2, 3) for x in (3, 4, 5)}
    assert set(np.flatnonzero(np.isnan(t).all(axis=1)).tolist()) == want and set(np.flatnonzero(np.isnan(t).any(axis=1)).tolist()) == want
    # infinities outside the support do not reach the pixel either (0 * inf would be NaN)
    dirty[2 * 9 + 4, 0, :] = np.inf
    m = host.filter_frame(dirty, 9, 5, sp, Filter.mitchell(2.0))
    far = [i for i in range(45) if abs(i % 9 - 4) > 1 or abs(i // 9 - 2) > 1]
    assert np.isfinite(m[far]).all() and not np.isfinite(m[2 * 9 + 4]).any()


# ---- API and mirrors ---------------------------------------------------------------------------------------------------------------
def test_validation_through_c(host):
    lib = host.lib
    samples, out = np.zeros((6, 4, 3)), np.zeros((6, 3))
    spc = SamplingC(2, 0, 0, 0.0, 1.0)

    def code(kind=1, radius=1.5, alpha=0.0, sp=spc, hsize=3, vsize=2):
        return lib.rtc_filter_frame(None, hsize, vsize, C.byref(sp), C.byref(FilterC(kind, 0, radius, alpha)), samples.ctypes.data, out.ctypes.data)
    assert code() == 0 and code(kind=0, radius=0.5) == 0 and code(kind=2, alpha=2.0) == 0 and code(kind=3, radius=3.0) == 0
    assert code(kind=4) == 1 and code(kind=-1) == 1                                        # RTC_ERR_INVALID
    assert code(radius=0.49) == 1 and code(radius=math.nan) == 1 and code(radius=math.inf) == 1 and code(radius=-1.0) == 1
    assert code(kind=2, alpha=0.0) == 1 and code(kind=2, alpha=-1.0) == 1 and code(kind=2, alpha=math.nan) == 1 and code(kind=2, alpha=math.inf) == 1
    assert code(kind=1, alpha=math.nan) == 0 and code(kind=3, alpha=-1.0) == 0             # alpha is the Gaussian's alone
    assert code(radius=3.5) == 2 and b"radius" in lib.rtc_last_error()                     # RTC_ERR_UNSUPPORTED
    assert code(sp=SamplingC(0, 0, 0, 0.0, 1.0)) == 1 and code(sp=SamplingC(17, 0, 0, 0.0, 1.0)) == 2 and code(sp=SamplingC(2, 2, 0, 0.0, 1.0)) == 1
    assert code(hsize=0) == 1 and code(vsize=0) == 1
    fl = FilterC(1, 0, 1.5, 0.0)
    assert lib.rtc_filter_frame(None, 3, 2, None, C.byref(fl), samples.ctypes.data, out.ctypes.data) == 1      # NULL arguments
    assert lib.rtc_filter_frame(None, 3, 2, C.byref(spc), None, samples.ctypes.data, out.ctypes.data) == 1
    assert lib.rtc_filter_frame(None, 3, 2, C.byref(spc), C.byref(fl), None, out.ctypes.data) == 1
    assert lib.rtc_filter_frame(None, 3, 2, C.byref(spc), C.byref(fl), samples.ctypes.data, None) == 1
    # the render entry points validate before they touch a device
    rc = ff.make_camera(scenes.cover(9, 5)[0])
    assert lib.rtc_render_filtered(None, C.byref(rc), C.byref(spc), C.byref(fl), 5, 0, 5, out.ctypes.data, None) == 1   # NULL scene
    assert lib.rtc_render_filtered_rgb8(None, C.byref(rc), C.byref(spc), C.byref(fl), 5, out.ctypes.data, None) == 1
    assert lib.rtc_render_filtered_rgb8(None, None, C.byref(spc), C.byref(fl), 5, out.ctypes.data, None) == 1


def test_validation_through_filter():
    assert Filter.box() == Filter("box", 0.5) and Filter.tent() == Filter("tent", 1.5)
    assert Filter.gaussian() == Filter("gaussian", 1.5, 2.0) and Filter.mitchell() == Filter("mitchell", 2.0)
    assert Filter.mitchell(3.0).radius == 3.0 and Filter.tent(2.0, ).alpha == 0.0
    for bad in (dict(kind="sinc", radius=1.0), dict(kind="box", radius=0.49), dict(kind="tent", radius=math.nan), dict(kind="tent", radius=math.inf),
                dict(kind="tent", radius=-2.0), dict(kind="mitchell", radius=3.5), dict(kind="box", radius="wide"),
                dict(kind="gaussian", radius=1.5, alpha=0.0), dict(kind="gaussian", radius=1.5, alpha=-1.0), dict(kind="gaussian", radius=1.5, alpha=math.nan),
                dict(kind="gaussian", radius=1.5, alpha=math.inf), dict(kind="gaussian", radius=1.5)):
        with pytest.raises(ValueError):
            Filter(**bad)
    Filter("tent", 1.5, alpha=math.nan)   # alpha is the Gaussian's alone
    with pytest.raises(Exception):
        Filter.box().radius = 2.0   # frozen
    c = FilterC.of(Filter.gaussian(2.5, 0.75))
    assert (c.kind, c.radius, c.alpha) == (2, 2.5, 0.75) and C.sizeof(FilterC) == 24
    assert [FilterC.of(f).kind for f in filters(1.0)] == [0, 1, 2, 3] and FILTER_KINDS == ("box", "tent", "gaussian", "mitchell")
    # the rules of par_render that need no library
    cam, world = scenes.chapter11_glass_air_bubble(8, 8)
    with pytest.raises(ValueError):
        Image.par_render(cam, world, adaptive=Adaptive(Sampling(), Sampling(side=2), 0.1), filter=Filter.tent())


def test_libraries_without_the_entry_points_refuse(emu, orc):
    cam, world = scenes.chapter11_glass_air_bubble(8, 8)
    for be in (emu, orc):
        nw = be.build_world(world)
        with pytest.raises(RtwError):
            be.render_filtered(nw, cam, Sampling(side=2), Filter.tent())
        with pytest.raises(RtwError):
            be.filter_frame(np.zeros((64, 4, 3)), 8, 8, Sampling(side=2), Filter.tent())
        with pytest.raises(RtwError):
            Image.par_render(cam, world, backend=be, filter=Filter.tent())
        with pytest.raises(RtwError):
            Image.par_render(cam, world, backend=be, sampling=Sampling(side=2), filter=Filter.mitchell())
    assert Image.par_render(cam, world, fuel=1, backend=emu).pixels.shape == (64, 3)   # None takes today's route


def test_exports_and_rust_mirror():
    lib = load(LIB)
    names = ("rtc_render_filtered", "rtc_render_filtered_rgb8", "rtc_filter_frame")
    for name in names:
        assert hasattr(lib, name), name
    h = open(os.path.join(ROOT, "include", "rtc.h")).read()
    rs = open(os.path.join(ROOT, "shim", "gpu.rs")).read()
    c, r = c_struct(h, "rtc_filter"), rust_struct(rs, "RtcFilter")
    assert c == r == [("kind", "i32", 0), ("_pad", "u32", 0), ("radius", "f64", 0), ("alpha", "f64", 0)]
    assert "RTC_FILTER_BOX = 0, RTC_FILTER_TENT = 1, RTC_FILTER_GAUSSIAN = 2, RTC_FILTER_MITCHELL = 3" in h
    for k, name in enumerate(("BOX", "TENT", "GAUSSIAN", "MITCHELL")):
        assert "pub const RTC_FILTER_%s: i32 = %d;" % (name, k) in rs
    assert "#define RTC_FILTER_MAX_RADIUS 3.0" in h and "pub const RTC_FILTER_MAX_RADIUS: f64 = 3.0;" in rs
    for name in names:
        assert "fn %s(" % name in rs, name
