"""The device against the extended oracle (oracle/rt_oracle_ext.hpp: area lights, texture maps, light cones, the background and bump
records restated from include/rtc.h) on full ray trees, both device paths: every primary hit and every hit-tree digest bit-exact, the
NaN / infinity pattern equal, colours within RGB_TOL.  Pixels and rays whose tie flag is set (a (u, v) decision behind atan2 / acos within 1e-9 of its threshold;
test_oracle_ext_cpu.py caps their share at 2 %) are left out of the colour comparison alone.  One oracle pass per scene, shared by both
paths.  Largest |dRGB| measured on an MI355X per case: DESIGN.md, "The extended oracle"."""
import numpy as np
import pytest

import ext_cases as ec
from oracle_ext_lib import oracle_ext
from parity import RGB_TOL, unmasked, assert_parity, assert_ray_parity_with_panics, rgb_error
from raytracer_challenge_amd.scene import Sampling

PATHS = ["1", "4"]


@pytest.fixture(scope="module")
def ext():
    return oracle_ext()


_REFS = {}


def reference(ext, key, world, cam, fuel):
    """(rgb, primary hits, digests) and the tie flags of one scene, from the ext oracle, once for both paths."""
    if key not in _REFS:
        nw = ext.build_world(world)
        _REFS[key] = (ext.render_with_digest(nw, cam, fuel), ext.pixel_ties(nw, cam, fuel))
    return _REFS[key]


@pytest.mark.gpu
@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("name", sorted(ec.FRAME_CASES))
def test_showcases_fixtures_and_the_everything_scene(hip, ext, name, path, monkeypatch):
    """The committed showcases and fixtures at fuel 5 (texture / spot / sky showcases at 96x54, the jittered penumbra and mirror worlds at
    96x64, the build matrix's uv scene under a background) and the scene that holds every extension at once, with a skybox and with a
    gradient over RTC_BG_DIRECTION, at 64x36 and at 13x7 (less than a wave wide, a multiple of nothing).  Bumped worlds (include/rtc.h
    rtc_bump; the oracle's steps 5-7 sit in rt_oracle.hpp's prepare_state): one scene per NP build (rtc_bump_info.trace_build 0..11) at 48x32, each asserted to
    run that row; the everything scene with a record on every material (one of amplitude 0); bump_showcase at 48x27; amplitude 2.0 on a
    glass-and-mirror sphere and a mirror plane, where a third of the hit pixels have ns . eye < 0."""
    cam, world, fuel = ec.frame_case(name)
    ref, tie = reference(ext, name, world, cam, fuel)
    monkeypatch.setenv("RTC_KERNEL", path)
    if name in ec.BUMPED_CASES:
        from test_bump_gpu import bump_info
        nw = hip.build_world(world)
        info = bump_info(hip, nw)
        assert info.has_bump == 1 and info.n_bumps >= 2, name
        if name.startswith("np_row_"):
            row = int(name[-2:])
            assert info.trace_build == row and info.trace_bg == (1 if row >= 6 else 0) and info.wf_shade_build == info.trace_uv, (name, info.trace_build)
        nw.close()
    err = assert_parity(hip, ext, world, cam, fuel, label="%s path %s" % (name, path), ref=ref, color_mask=tie)
    print("ext parity: %s path %s: max |dRGB| = %.3e (%d of %d pixels flagged)" % (name, path, err, int(tie.sum()), tie.size))


@pytest.mark.gpu
@pytest.mark.parametrize("seed", ec.fuzz_seeds())
def test_seventh_fuzz_wave(hip, ext, seed, monkeypatch):
    """Worlds of the first two fuzz generators decorated from the seed: lights turned into area lights (1..4 x 1..4 steps, a 16x1 now
    and then, jittered or not), cones (open, hard, smooth, aimed away), UV patterns over all maps x record kinds on a fifth of the
    materials (some under Mixture or jitter nodes), a background (plain, Mixture, spherical UV, skybox)."""
    cam, world, fuel, label = ec.seventh_wave(seed)
    ref, tie = reference(ext, ("fuzz", seed), world, cam, fuel)
    for path in PATHS:
        monkeypatch.setenv("RTC_KERNEL", path)
        err = assert_parity(hip, ext, world, cam, fuel, label=label + " path " + path, ref=ref, color_mask=tie)
        print("ext parity: %s path %s: max |dRGB| = %.3e (%d flagged)" % (label, path, err, int(tie.sum())))


@pytest.mark.gpu
@pytest.mark.parametrize("seed", ec.bump_fuzz_seeds())
def test_eighth_fuzz_wave(hip, ext, seed, monkeypatch):
    """The seventh wave's worlds with a bump record on about a third of their materials, group and OBJ materials included: kinds uniform,
    amplitude from {0, 1e-300, 0.05, 0.3, 2.0}, frequency 10^U(-1, 1.5), octaves from {1, 3, 8}."""
    cam, world, fuel, label = ec.eighth_wave(seed)
    ref, tie = reference(ext, ("bumped fuzz", seed), world, cam, fuel)
    for path in PATHS:
        monkeypatch.setenv("RTC_KERNEL", path)
        err = assert_parity(hip, ext, world, cam, fuel, label=label + " path " + path, ref=ref, color_mask=tie)
        print("ext parity: %s path %s: max |dRGB| = %.3e (%d flagged)" % (label, path, err, int(tie.sum())))


@pytest.mark.gpu
@pytest.mark.parametrize("name", ec.BUMP_RAY_WORLDS)
def test_ray_sets_through_trace_rays_on_bumped_worlds(hip, ext, name, monkeypatch):
    """rtc_trace_rays (the NP builds over explicit rays) on the bumped everything scene, the bumped open world and a rippled mirror plane
    of frequency 1 under a transform of powers of two, once bare (the kplanes shortcut of prepare_state) and once under a transformed
    group: cases.edge_rays, cases.special_rays (cone and cylinder apexes hand a NaN geometric normal to step 4), rays that start inside
    a bumped glass sphere, and rays that land at material-space radius exactly 0 (r == 0), 0.5 (g == 1) and 1.0 (g == 0)."""
    world, fuel, sets = ec.bump_ray_sets(name)
    nw = ext.build_world(world)
    for which, rays in sets.items():
        tie = ext.ray_ties(nw, rays, fuel)
        for path in PATHS:
            monkeypatch.setenv("RTC_KERNEL", path)
            err, panics = assert_ray_parity_with_panics(hip, ext, world, rays, fuel, label="bumped %s %s rays, path %s" % (name, which, path), color_mask=tie)
            print("ext parity: bumped %s %s rays path %s: max |dRGB| = %.3e (%d rays, %d panic, %d flagged)" % (name, which, path, err, len(rays), panics, int(tie.sum())))


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["shared_material", "group_material", "many_materials", "second_set_bump"])
def test_the_flattener_puts_each_record_on_its_primitives(hip, ext, name):
    """rtc_bump_normals reads, per primitive, the record and the material_inv the product's flattener interned for it: equal, bit for bit,
    to what the oracle's world holds for that primitive (which test_oracle_ext_cpu.py holds to the answer written down) for two shapes
    sharing a material but not the bump, a group's material replacing its children's records, a second rtw_element_set_bump call, and
    300 materials with a record on every odd one (material rows past 255)."""
    import build_matrix as bm
    from oracle_ext_lib import world_with_two_set_bump_calls
    from raytracer_challenge_amd.scene import Matrix
    from test_oracle_ext_cpu import bits, flatten_items
    lib = hip.lib
    if name == "second_set_bump":
        t = Matrix.translation(1.0, -2.0, 0.5).flat()
        nw, nwo = (world_with_two_set_bump_calls(b, (1, 5, 0.3, 2.0), (2, 0, 0.2, 1.5), t) for b in (hip, ext))
        n_prims = 1
    else:
        world, want = ec.flatten_worlds()[name]
        nw, nwo, n_prims = hip.build_world(world), ext.build_world(world), len(want)
    assert nw.primitive_count == n_prims == nwo.primitive_count
    prims, points, normals = flatten_items(n_prims)
    out = np.full((len(prims), 3), np.nan)
    assert lib.rtc_bump_normals(bm.scene_of(hip, nw), prims.ctypes.data, points.ctypes.data, normals.ctypes.data, len(prims), out.ctypes.data) == 0, lib.rtc_last_error()
    want_n = ext.world_bump_normals(nwo, prims, points, normals)
    differ = (bits(out) != bits(want_n)).any(axis=1)
    assert not differ.any(), "%s: %d of %d items differ, first primitives %s" % (name, int(differ.sum()), len(prims), prims[differ][:5])
    assert (bits(out) != bits(normals)).any()


def sampled_parity(hip, ext, path, world, what):
    cam = ec.everything_camera(24, 16)
    sp = Sampling(side=2, jitter=True, seed=2024, lens_radius=0.08, focal_distance=7.0)
    nw = hip.build_world(world)
    rays = hip.camera_rays(cam, sp, nw=nw)
    assert rays.shape == (24 * 16, 4, 6)
    key = ("sampled", what, rays.tobytes())
    if key not in _REFS:
        nwo = ext.build_world(world)
        _REFS[key] = (ext.color_at(nwo, rays.reshape(-1, 6), 5)[0].reshape(-1, 4, 3), ext.ray_ties(nwo, rays.reshape(-1, 6), 5).reshape(-1, 4).any(axis=1))
    colours, tie = _REFS[key]
    want = colours[:, 0]
    for k in range(1, 4):
        want = want + colours[:, k]
    want = want / 4.0
    got = hip.render_sampled(nw, cam, sp, 5)
    err = rgb_error(*unmasked(got, want, tie), "sampled camera, %s, path %s" % (what, path))
    print("ext parity: sampled camera over the %s path %s: max |dRGB| = %.3e (%d of %d pixels flagged)" % (what, path, err, int(tie.sum()), tie.size))
    assert err <= RGB_TOL
    assert tie.mean() <= 0.02


@pytest.mark.gpu
@pytest.mark.parametrize("path", PATHS)
def test_sampled_camera_over_the_bumped_everything_scene(hip, ext, path, monkeypatch):
    """The bumped twin of the test below: rtc_render_sampled launches the NP builds over explicit rays in another pixel-map mode."""
    monkeypatch.setenv("RTC_KERNEL", path)
    sampled_parity(hip, ext, path, ec.bumped_everything_world(True), "bumped everything scene")


@pytest.mark.gpu
@pytest.mark.parametrize("seed", ec.RAY_SEEDS)
def test_ray_sets_through_trace_rays(hip, ext, seed, monkeypatch):
    """rtc_trace_rays over three of the wave's worlds: cases.edge_rays (axis-parallel and non-unit directions, which RTC_BG_DIRECTION
    takes as they are; exact diagonals and a NaN component for the cube face rule) and cases.special_rays.  Rays the reference panics on
    are refused singly by the device, as ever."""
    world, fuel, label, sets = ec.ray_sets(seed)
    nw = ext.build_world(world)
    for name, rays in sets.items():
        tie = ext.ray_ties(nw, rays, fuel)
        for path in PATHS:
            monkeypatch.setenv("RTC_KERNEL", path)
            err, panics = assert_ray_parity_with_panics(hip, ext, world, rays, fuel, label="%s %s rays, path %s" % (label, name, path), color_mask=tie)
            print("ext parity: %s %s rays path %s: max |dRGB| = %.3e (%d rays, %d panic, %d flagged)" % (label, name, path, err, len(rays), panics, int(tie.sum())))


@pytest.mark.gpu
@pytest.mark.parametrize("path", PATHS)
def test_sampled_camera_over_the_everything_scene(hip, ext, path, monkeypatch):
    """rtc_render_sampled's pixel is the mean, in k order, of the ext oracle's World::color_at over rtc_camera_rays' rays: 2x2 jittered
    samples through a thin lens, 24x16."""
    monkeypatch.setenv("RTC_KERNEL", path)
    sampled_parity(hip, ext, path, ec.everything_world(True), "everything scene")
