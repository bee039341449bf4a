"""The device's ray counters -- the numerator of every rays-per-second figure bench.py prints -- against the oracle's count of the
de-duplicated ray tree (oracle_capi.cpp orc_ray_counts; test_ray_counts_cpu.py ties that count to the reference's recursion and to
numbers written down by hand), on both device paths.  Every comparison is exact equality of `pixels` and the five ray counters: no
tolerance, no excluded pixel or ray.  One oracle pass per case, shared by both paths.  Totals as measured on an MI355X: DESIGN.md,
"What counts as a ray"."""
import ctypes as C

import numpy as np
import pytest

import build_matrix as bm
import cases
import ext_cases as ec
import foreign_flattener as ff
import ray_counts as rc
import wf_shade_queues as wq
from oracle_ext_lib import oracle_ext
from raytracer_challenge_amd import scenes
from raytracer_challenge_amd.device import RtcStatsC
from raytracer_challenge_amd.scene import Adaptive, Camera, Filter, Matrix, Sampling, Shutter, Vector

pytestmark = pytest.mark.gpu
PATHS = ["1", "4"]
vp = C.c_void_p


@pytest.fixture(scope="module")
def ext():
    return oracle_ext()


_WANT = {}


def want_of(key, make):
    """The oracle's answer for `key`, computed once for both paths."""
    if key not in _WANT:
        _WANT[key] = make()
    return _WANT[key]


def frame_want(lib, key, world, cam, fuel):
    return want_of(key, lambda: rc.expected(lib.ray_counts(lib.build_world(world), cam, fuel), cam.hsize * cam.vsize))


def show(label, st):
    print("ray counts: %s: %s" % (label, " ".join("%s=%d" % (k, v) for k, v in rc.as_counts(st).items())))


# ---- 1. totals per class ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("name", sorted(rc.PLAIN_CASES))
def test_plain_scenes(hip, orc, name, path, monkeypatch):
    """The cover, chapter 11's glass bubble, the low teapot (the one-kernel path answers a light behind the surface without a traversal:
    the ray is counted all the same), nested_glass and glass_cluster, at fuel 5."""
    monkeypatch.setenv("RTC_KERNEL", path)
    cam, world, fuel = rc.PLAIN_CASES[name]()
    st = rc.render_stats(hip, hip.build_world(world), cam, fuel)
    show("%s path %s" % (name, path), st)
    rc.assert_counts(st, frame_want(orc, name, world, cam, fuel), "%s path %s" % (name, path))


@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("name", sorted(rc.EXT_CASES))
def test_extension_scenes(hip, ext, name, path, monkeypatch):
    """Area lights (one shadow ray per sample), cones (none for a sample whose factor is 0.0), backgrounds (a miss adds nothing), bumps
    (total internal reflection decided on the shading normal): the jittered penumbra and mirror worlds, the spot and sky showcases, the
    scene that holds every extension with a skybox and with a gradient, its bumped twin, the steep-bump scene."""
    monkeypatch.setenv("RTC_KERNEL", path)
    cam, world, fuel = rc.EXT_CASES[name]()
    st = rc.render_stats(hip, hip.build_world(world), cam, fuel)
    show("%s path %s" % (name, path), st)
    rc.assert_counts(st, frame_want(ext, name, world, cam, fuel), "%s path %s" % (name, path))


@pytest.mark.parametrize("wave,seed", [(w, s) for w in sorted(rc.FUZZ_SEEDS) for s in rc.FUZZ_SEEDS[w]])
def test_fuzz_worlds(hip, orc, ext, wave, seed, monkeypatch):
    """Four seeds each of the first, seventh and eighth fuzz waves."""
    cam, world, fuel, which = rc.fuzz_case(wave, seed)
    want = frame_want(orc if which == "plain" else ext, (wave, seed), world, cam, fuel)
    for path in PATHS:
        monkeypatch.setenv("RTC_KERNEL", path)
        st = rc.render_stats(hip, hip.build_world(world), cam, fuel)
        show("%s wave seed %d path %s" % (wave, seed, path), st)
        rc.assert_counts(st, want, "%s wave seed %d path %s" % (wave, seed, path))


# ---- 2. per depth, by differencing -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("path", PATHS)
def test_the_difference_between_two_fuels_is_one_depth(hip, orc, path, monkeypatch):
    """The rays at depth d do not depend on the fuel once fuel >= d: totals(fuel f) - totals(fuel f - 1) are the oracle's reflect[f],
    refract[f] and shadow[f] of its fuel-4 run, fuel 0 is depth 0.  A hit at the last level has no fuel left and needs no n1 / n2: the
    container difference is the oracle's container[f - 1]."""
    monkeypatch.setenv("RTC_KERNEL", path)
    cam, world = rc.two_light_glass_and_mirror()
    deep = want_of("by depth", lambda: orc.ray_counts(orc.build_world(world), cam, 4))
    nw = hip.build_world(world)
    got = [rc.as_counts(rc.render_stats(hip, nw, cam, f)) for f in range(5)]
    rc.assert_counts(got[4], rc.expected(deep, cam.hsize * cam.vsize), "fuel 4, path " + path)
    assert all(int(deep[k][d]) > 0 for k in ("reflect", "refract", "shadow") for d in range(1, 5))
    assert got[0]["rays_shadow"] == int(deep["shadow"][0]) and got[0]["rays_reflect"] == got[0]["rays_refract"] == got[0]["rays_container"] == 0
    for f in range(1, 5):
        for key in ("reflect", "refract", "shadow"):
            assert got[f]["rays_" + key] - got[f - 1]["rays_" + key] == int(deep[key][f]), (key, f, path)
        assert got[f]["rays_container"] - got[f - 1]["rays_container"] == int(deep["container"][f - 1]), (f, path)
        assert got[f]["pixels"] == got[f]["rays_primary"] == cam.hsize * cam.vsize


# ---- 3. every entry point that fills an rtc_stats --------------------------------------------------------------------------------------
def glass_scene():
    cam, world = scenes.chapter11_glass_air_bubble(37, 19)     # neither side a multiple of 8: no whole tile, no whole wave
    return cam, world


@pytest.mark.parametrize("path", PATHS)
def test_rtc_render_over_a_range_a_sub_range_and_a_list(hip, ext, path, monkeypatch):
    monkeypatch.setenv("RTC_KERNEL", path)
    cam, world = ec.everything_camera(24, 16), ec.everything_world(True)
    nw = hip.build_world(world)
    nwo = want_of("everything oracle world", lambda: ext.build_world(world))
    n = cam.hsize * cam.vsize
    idx = np.random.default_rng(11).integers(0, n, 203).astype(np.uint64)
    idx[100:120] = idx[3]                                                      # repeats: a pixel listed twice is traced and counted twice
    for what, kw, pixels in (("range", {}, np.arange(n)), ("sub-range", dict(first=29, n=157), np.arange(29, 29 + 157)), ("list", dict(pixel_indices=idx), idx)):
        want = want_of(("render", what), lambda: rc.expected(ext.ray_counts(nwo, cam, 5, pixels), len(pixels)))
        rc.assert_counts(rc.render_stats(hip, nw, cam, 5, **kw), want, "rtc_render %s path %s" % (what, path))


@pytest.mark.parametrize("path", PATHS)
def test_rgb8_rows_and_bands(hip, ext, path, monkeypatch):
    """rtc_render_rgb8 over the frame; rtc_render_rows_device over part 1 of 3 (rows 1, 4, ...) and rtc_render_bands_device over part 0
    of 3 in bands of 4 rows (the first band and the last one, which is short), counting."""
    import torch
    monkeypatch.setenv("RTC_KERNEL", path)
    cam, world = ec.everything_camera(24, 14), ec.everything_world(False)
    nw = hip.build_world(world)
    nwo = want_of("gradient oracle world", lambda: ext.build_world(world))
    n = cam.hsize * cam.vsize
    rc.assert_counts(rc.rgb8_stats(hip, nw, cam, 5), want_of("rgb8", lambda: rc.expected(ext.ray_counts(nwo, cam, 5), n)), "rtc_render_rgb8 path " + path)
    out = torch.empty(n * 3, dtype=torch.float64, device="cuda")
    for band, part, owned in ((1, 1, [1, 4, 7, 10, 13]), (4, 0, [0, 1, 2, 3, 12, 13])):
        rows = rc.band_rows_of(cam.vsize, band, part, 3)
        assert rows == owned and len(rows) == hip.lib.rtc_band_rows_owned(cam.vsize, band, part, 3)
        pixels = rc.rows_pixels(cam, rows)
        want = want_of(("bands", band), lambda: rc.expected(ext.ray_counts(nwo, cam, 5, pixels), len(pixels)))
        rc.assert_counts(rc.bands_stats(hip, nw, cam, 5, band, part, 3, len(rows), vp(out.data_ptr())), want, "bands of %d rows, path %s" % (band, path))


@pytest.mark.parametrize("path", PATHS)
def test_rtc_render_multi_sums_its_replicas(hip, orc, path, monkeypatch):
    """Two replicas on one device, each with the bands it owns: the sum is the frame's count, once."""
    monkeypatch.setenv("RTC_KERNEL", path)
    lib = hip.lib
    cam, world = glass_scene()
    desc = ff.flatten(world).desc()
    m, devs = vp(), (C.c_int * 2)(0, 0)
    assert lib.rtc_multi_create(C.byref(desc), devs, 2, C.byref(m)) == 0, hip._err()
    try:
        cam_c, st, rgb = ff.make_camera(cam), RtcStatsC(), np.empty((cam.hsize * cam.vsize, 3))
        assert lib.rtc_render_multi(m, C.byref(cam_c), 5, rgb.ctypes.data, C.byref(st)) == 0, hip._err()
    finally:
        lib.rtc_multi_destroy(m)
    rc.assert_counts(st, frame_want(orc, "glass 37x19", world, cam, 5), "rtc_render_multi path " + path)


def _ray_sets():
    cam, world = cases.nested_glass()
    plain = {"edge": cases.edge_rays(768), "special": cases.special_rays(world, 512)}
    ext_world, fuel, _, sets = ec.ray_sets(80001)
    return (world, 3, plain), (ext_world, fuel, {k: v[:768] for k, v in sets.items()})


@pytest.mark.parametrize("path", PATHS)
def test_rtc_trace_rays_on_the_edge_and_special_ray_sets(hip, orc, ext, path, monkeypatch):
    """cases.edge_rays and cases.special_rays on nested_glass and on a world of the seventh fuzz wave.  Rays on which the reference
    panics are refused by the device and have no count; the oracle finds them (build_matrix.panic_free) and they are left out of both
    sides' input."""
    monkeypatch.setenv("RTC_KERNEL", path)
    for lib, (world, fuel, sets) in zip((orc, ext), _ray_sets()):
        nw = hip.build_world(world)
        for which, rays in sets.items():
            def make():
                keep = rays[bm.panic_free(lib, world, rays, fuel)]
                return keep, rc.expected(lib.ray_counts_rays(lib.build_world(world), keep, fuel), len(keep))
            keep, want = want_of(("rays", lib.name, which), make)
            assert len(keep) > 0.9 * len(rays)
            rc.assert_counts(rc.trace_stats(hip, nw, keep, fuel), want, "rtc_trace_rays %s %s path %s" % (lib.name, which, path))


SAMPLING = Sampling(side=2, jitter=True, seed=2024, lens_radius=0.08, focal_distance=7.0)


def sampled_want(hip, ext, nwo, cam, sp, fuel, pixels=None):
    """The oracle's count over the rays rtc_camera_rays returns (host evaluation; test_sampled_camera_*.py hold them to the numpy
    restatement and to the device's generator)."""
    rays = hip.camera_rays(cam, sp, pixel_indices=pixels)
    return rc.expected(ext.ray_counts_rays(nwo, rays.reshape(-1, 6), fuel), rays.shape[0])


@pytest.mark.parametrize("path", PATHS)
def test_rtc_render_sampled_in_one_chunk_and_in_several(hip, ext, path, monkeypatch):
    monkeypatch.setenv("RTC_KERNEL", path)
    cam, world = ec.everything_camera(24, 16), ec.everything_world(True)
    nw = hip.build_world(world)
    nwo = want_of("everything oracle world", lambda: ext.build_world(world))
    want = want_of("sampled", lambda: sampled_want(hip, ext, nwo, cam, SAMPLING, 5))
    assert want["rays_primary"] == 4 * 24 * 16
    monkeypatch.delenv("RTC_SAMPLED_MAX_RAYS", raising=False)
    rc.assert_counts(rc.sampled_stats(hip, nw, cam, SAMPLING, 5), want, "rtc_render_sampled, one chunk, path " + path)
    monkeypatch.setenv("RTC_SAMPLED_MAX_RAYS", "300")             # three rows of 96 rays per chunk: six chunks, the last one short
    rc.assert_counts(rc.sampled_stats(hip, nw, cam, SAMPLING, 5), want, "rtc_render_sampled, several chunks, path " + path)


@pytest.mark.parametrize("path", PATHS)
def test_rtc_render_adaptive_counts_both_passes(hip, ext, path, monkeypatch):
    """The base pass over every pixel plus the fine pass over the pixels of the returned mask."""
    monkeypatch.setenv("RTC_KERNEL", path)
    monkeypatch.delenv("RTC_SAMPLED_MAX_RAYS", raising=False)
    cam, world = ec.everything_camera(24, 16), ec.everything_world(True)
    nw = hip.build_world(world)
    nwo = want_of("everything oracle world", lambda: ext.build_world(world))
    ad = Adaptive(Sampling(), SAMPLING, 0.1)
    st, mask = rc.adaptive_stats(hip, nw, cam, ad, 5)
    refined = np.flatnonzero(mask).astype(np.uint64)
    assert 16 < len(refined) < mask.size - 16
    base = want_of("adaptive base", lambda: sampled_want(hip, ext, nwo, cam, ad.base, 5))
    fine = want_of(("adaptive fine", refined.tobytes()), lambda: sampled_want(hip, ext, nwo, cam, ad.fine, 5, refined))
    want = rc.add(base, fine)
    want["pixels"] = mask.size
    assert want["rays_primary"] == mask.size + 4 * len(refined)
    rc.assert_counts(st, want, "rtc_render_adaptive path " + path)


@pytest.mark.parametrize("path", PATHS)
def test_rtc_render_filtered_counts_the_traced_rows(hip, ext, path, monkeypatch):
    """A row range traces its halo rows too (include/rtc.h: rows [max(0, a - W), min(vsize, b + W)) of a chunk [a, b)); with one output
    row per chunk every chunk traces its own halo again."""
    from test_filter_cpu import window
    monkeypatch.setenv("RTC_KERNEL", path)
    cam, world = ec.everything_camera(24, 16), ec.everything_world(True)
    nw = hip.build_world(world)
    nwo = want_of("everything oracle world", lambda: ext.build_world(world))
    sp, flt = Sampling(side=2, jitter=True, seed=7), Filter.tent(1.5)
    W = window(flt.radius)
    assert W == 1

    def rows_want(a, b):
        return want_of(("filtered rows", a, b), lambda: sampled_want(hip, ext, nwo, cam, sp, 5, rc.rows_pixels(cam, range(max(0, a - W), min(cam.vsize, b + W)))))

    monkeypatch.delenv("RTC_SAMPLED_MAX_RAYS", raising=False)
    want = dict(rows_want(0, cam.vsize), pixels=cam.hsize * cam.vsize)
    rc.assert_counts(rc.filtered_stats(hip, nw, cam, sp, flt, 5), want, "rtc_render_filtered, the frame, path " + path)
    want = dict(rows_want(5, 8), pixels=3 * cam.hsize)
    rc.assert_counts(rc.filtered_stats(hip, nw, cam, sp, flt, 5, 5, 3), want, "rtc_render_filtered, rows 5..7, path " + path)
    monkeypatch.setenv("RTC_SAMPLED_MAX_RAYS", "1")
    want = dict(rc.add(*[rows_want(y, y + 1) for y in range(cam.vsize)]), pixels=cam.hsize * cam.vsize)
    rc.assert_counts(rc.filtered_stats(hip, nw, cam, sp, flt, 5), want, "rtc_render_filtered, a chunk per row, path " + path)


@pytest.mark.parametrize("path", PATHS)
def test_rtc_render_shutter_sums_its_poses(hip, ext, path, monkeypatch):
    """Three poses -- the everything scene with its ball moved, seen from a moving camera: the sum over the poses of the oracle's count of
    the rays dealt to each pose (the restated dealing of test_shutter_cpu.py), in that pose's world."""
    import dataclasses
    from test_shutter_cpu import poses_of
    monkeypatch.setenv("RTC_KERNEL", path)
    monkeypatch.delenv("RTC_SAMPLED_MAX_RAYS", raising=False)
    base = ec.everything_world(False)
    worlds, cams = [], []
    for p in range(3):
        ball = base.elements[1]
        moved = dataclasses.replace(ball, args=dataclasses.replace(ball.args, transform=Matrix.translation(0.25 * p, 0.0, 0.0) * ball.args.transform))
        worlds.append(type(base)(base.lights, [base.elements[0], moved] + list(base.elements[2:]), base.background))
        cams.append(Camera.new(24, 16, 1.0, Camera.transform(Vector.point(0.3 + 0.1 * p, 2.6, -7.0), Vector.point(-0.2, 0.8, 0.0), Vector.vector(0.0, 1.0, 0.0))))
    sp, shutter = Sampling(side=2, jitter=True, seed=5), Shutter(hashed=True)
    n = 24 * 16

    def make():
        pose = poses_of(sp, True, 3, list(range(n))).reshape(n, sp.samples)
        wants = []
        for p in range(3):
            rays = hip.camera_rays(cams[p], sp)[pose == p]
            assert len(rays) > 0
            wants.append(rc.expected(ext.ray_counts_rays(ext.build_world(worlds[p]), rays, 5), 0))
        return dict(rc.add(*wants), pixels=n)
    want = want_of("shutter", make)
    assert want["rays_primary"] == 4 * n
    st = RtcStatsC()
    hip.render_shutter([hip.build_world(w) for w in worlds], cams, sp, shutter, 5, stats=st)
    rc.assert_counts(st, want, "rtc_render_shutter path " + path)


# ---- 4. queue edges of the wavefront path ------------------------------------------------------------------------------------------------
QUEUE_EDGES = [  # (scene of wf_shade_queues.py, camera, rays at level 1): one below, at and one above a multiple of wf_shade's block of 512 items and of a wave of 64
    ("plain_and_patterned", (39, 26), 1023), ("plain_and_patterned", (29, 35), 1024), ("plain_and_patterned", (44, 23), 1025),
    ("all_plain_glass", (21, 27), 575), ("all_plain_glass", (19, 20), 384), ("all_plain_glass", (16, 12), 193),
]


@pytest.mark.parametrize("scene,size,level1", QUEUE_EDGES)
def test_a_level_that_ends_at_a_block_edge_loses_and_adds_no_ray(hip, orc, scene, size, level1, monkeypatch):
    """A counter bumped outside its queue-capacity guard, or a ray dropped at a block's last slot, shows where a level's ray count sits at
    a multiple of the block.  The wavefront path must have rendered the frame itself (n_launches: no queue overflowed into the
    one-kernel path) and both paths must report the oracle's counts."""
    cam, world = wq.SCENES[scene]()
    cam = rc.resized(cam, *size)
    deep = orc.ray_counts(orc.build_world(world), cam, 5)
    assert int(deep["reflect"][1] + deep["refract"][1]) == level1
    for path in PATHS:
        monkeypatch.setenv("RTC_KERNEL", path)
        st = rc.render_stats(hip, hip.build_world(world), cam, 5)
        assert st.n_launches == (2 * 5 + 4 if path == "4" else 1), (path, st.n_launches)
        rc.assert_counts(st, rc.expected(deep, cam.hsize * cam.vsize), "%s %dx%d path %s" % (scene, size[0], size[1], path))
