"""Light-grid cells built from primitive silhouettes (scene_build.hpp build_light_grids): inside the rectangle that a
primitive's world box projects to on a face of a light's cube map, the primitive is entered only into the cells that the outline of a
convex polytope around it touches.  The lists must stay supersets of what any shadow ray of the cell can hit (checked by brute force
through the library's builder hook, include/rtc.h rtc_light_grid_build_raw), keep their structure, really get shorter, and change no
pixel, hit record or ray count on either device path."""
import os

import numpy as np
import pytest

import light_grid_cases as lg
from light_grid_cases import both_ways, lights_inside_scene
from parity import assert_parity
from raytracer_challenge_amd import scenes
from raytracer_challenge_amd.backend import Backend
from raytracer_challenge_amd.device import DeviceRenderer

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "raytracer_challenge_amd", "csrc", "librtc_amd.so")
CASES = lg.cases()

# Item count of the tight lists over the rectangle lists on config 2's scene (512 primitives, its two lights, n = 256), measured on the
# CPU through the hook: 0.4657 (profiles/light_grid_silhouettes.txt).  The bound is the midpoint between that and 1: a construction
# that falls back to the rectangle everywhere (ratio 1) fails.
MEASURED_RATIO = 0.4657
RATIO_BOUND = 0.5 * (MEASURED_RATIO + 1.0)


@pytest.fixture(scope="module")
def lib():
    """librtc_amd.so without a device: loading it and the host-only entry points need none."""
    return Backend(LIB).lib


@pytest.fixture(scope="module")
def emu():
    from emu_lib import emu as _emu
    return _emu()


# ---- 1. superset, by brute force ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [8, 64, 256])
@pytest.mark.parametrize("name", sorted(CASES))
def test_every_primitive_a_shadow_ray_can_hit_is_in_its_cell(lib, name, n):
    """~20 000 directions per case; along each, the ray from REACH away towards the light is put to the exact test of EVERY primitive
    (numpy f64 restatement of prim_hits): a primitive reporting any t in [0, REACH) must be listed in the direction's cell, with a
    distance bound no larger than the hit's distance from the light, unless the cell is left to the BVH walk.  The only (primitive,
    ray) pairs left out are those no BVH leaf serves either: a cone's rays with |a| < EPSILON (csrc/rtc_device.hpp visit_prim)."""
    prims, light, extra = CASES[name]
    rc, g = lg.build_raw(lib, prims, light, n)
    assert rc == 0, lib.rtc_last_error()
    rng = np.random.default_rng(7 + n)
    d = lg.directions(prims, light, n, rng, extra)
    assert len(d) >= 19000
    org = np.asarray(light) - lg.REACH * d
    cell = lg.cell_of(d, n)
    member, dmin = g.member()
    listed, bound, walk = member[cell], dmin[cell], g.walk[cell]
    hits = 0
    for k, p in enumerate(prims):
        t, unserved = lg.prim_hits(p, org, d)
        with np.errstate(invalid="ignore"):
            hit = (t >= 0.0) & (t < lg.REACH)
        hit[unserved] = False
        any_hit = hit.any(axis=1) & ~walk
        hits += int(any_hit.sum())
        missing = any_hit & ~listed[:, k]
        assert not missing.any(), "%s n %d: primitive %d (kind %d) is hit along %r but not in cell %d" % (name, n, k, p.kind, d[missing][0].tolist(), cell[missing][0])
        far = np.where(hit, lg.REACH - t, np.inf).min(axis=1)                  # the hit nearest to the light
        late = any_hit & (bound[:, k].astype(np.float64) > far * (1.0 + 1e-6) + 1e-30)
        assert not late.any(), "%s n %d: primitive %d: distance bound above a hit's distance" % (name, n, k)
    assert hits > 2000, hits                                                    # the rays do meet the primitives


# ---- 2. structure -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [8, 64, 256])
@pytest.mark.parametrize("name", sorted(CASES))
def test_list_structure_and_subset_of_the_rectangle_lists(lib, name, n):
    prims, light, _ = CASES[name]
    rc, tight = lg.build_raw(lib, prims, light, n, tight=1)
    rc0, rect = lg.build_raw(lib, prims, light, n, tight=0)
    assert rc == 0 and rc0 == 0
    for g in (tight, rect):
        c = g.cells.astype(np.int64)
        assert c[0] == 0 and c[-1] == len(g.ref) and (np.diff(c) >= 0).all()                       # offsets are monotone
        same = g.cell_of_item[1:] == g.cell_of_item[:-1]                                            # consecutive items of one cell:
        d0, d1, p0, p1 = g.dmin[:-1], g.dmin[1:], g.prim[:-1], g.prim[1:]
        assert (~same | (d0 < d1) | ((d0 == d1) & (p0 < p1))).all()                                 # sorted by (dmin, primitive), no primitive twice
        assert (np.diff(c)[g.walk] == 1).all()                                                      # an over-full cell holds the one marker
        assert ((g.prim >= 0) & (g.prim < len(prims)))[g.ref != lg.WALK].all()
    mt, dt = tight.member()
    mr, dr = rect.member()
    assert not (tight.walk & ~rect.walk).any()            # over-full cells only ever turn into listed cells, never the reverse
    keep = ~rect.walk
    assert not (mt[keep] & ~mr[keep]).any()               # every tight list is a subset of the rectangle list of its cell
    assert (dt[mt & mr] == dr[mt & mr]).all()             # with the same distance bounds
    assert mt[keep].sum() <= mr[keep].sum()


def test_hook_reports_errors_instead_of_crashing(lib):
    prims, light, _ = CASES["light_on_a_body_diagonal"]
    rc, g = lg.build_raw(lib, prims, light, 8)
    assert rc == 0
    rc, _ = lg.build_raw(lib, prims, light, 8, items_cap=len(g.ref) - 1)
    assert rc == 1 and b"capacity" in lib.rtc_last_error()
    assert lg.build_raw(lib, prims, light, 1)[0] == 1 and lg.build_raw(lib, prims, light, 513)[0] == 1
    unbounded = prims + [lg.cylinder(np.eye(4), -np.inf, 1.0, False)]
    assert lg.build_raw(lib, unbounded, light, 8)[0] == 1 and b"bounds" in lib.rtc_last_error()
    assert lib.rtc_light_grid_build_raw(None, None, None, None, 3, None, 8, 8, 1, None, 0, None, 0, None) == 1
    # a light in the middle of large primitives: over the work budget, the build declines
    big = [lg.sphere(lg.S(6.0)) for _ in range(80)]
    assert lg.build_raw(lib, big, (0.0, 0.0, 0.0), 8)[0] == -1


# ---- 3. tightness -------------------------------------------------------------------------------------------------------------------------
def test_tight_lists_are_shorter_on_the_benchmark_scene(lib):
    _, world = scenes.synthetic_analytic(n_primitives=512, seed=12345)
    prims = lg.world_prims(world)
    assert len(prims) == 512
    tight = rect = 0
    for light in world.lights:                         # (max_list 64: no cell of either build is left to the walk, the counts are the lists')
        o = light.origin[:3]
        rc1, g1 = lg.build_raw(lib, prims, o, 256, tight=1, max_list=64)
        rc0, g0 = lg.build_raw(lib, prims, o, 256, tight=0, max_list=64)
        assert rc1 == 0 and rc0 == 0
        assert not g0.walk.any() and not g1.walk.any()
        tight += len(g1.ref); rect += len(g0.ref)
    print("items: tight %d, rectangles %d, ratio %.4f" % (tight, rect, tight / rect))
    assert tight < rect
    assert tight / rect <= RATIO_BOUND, (tight, rect)


# ---- 4. results-neutral in the emulator ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cones,grouped", [(False, False), (True, True)])
def test_tight_lists_are_results_neutral_in_the_emulator(emu, orc, monkeypatch, cones, grouped):
    cam, world = scenes.synthetic_analytic(n_primitives=96, seed=7, cones=cones, grouped=grouped, hsize=96, vsize=54)
    both_ways(emu, world, cam, 3, monkeypatch)
    assert_parity(emu, orc, world, cam, 3, label="synthetic analytic, tight light grids")


def test_glass_cluster_in_the_emulator(emu, orc, monkeypatch):
    import cases
    cam, world = cases.glass_cluster()
    both_ways(emu, world, cam, 4, monkeypatch)
    for k in ("1", "4"):
        monkeypatch.setenv("RTC_KERNEL", k)
        assert_parity(emu, orc, world, cam, 4, label="glass cluster, tight light grids, path " + k)


def test_lights_inside_and_on_a_surface_in_the_emulator(emu, orc, monkeypatch):
    cam, world = lights_inside_scene()
    both_ways(emu, world, cam, 2, monkeypatch)
    assert_parity(emu, orc, world, cam, 2, label="lights inside bounds / on a surface, tight light grids")


def test_counters_in_the_emulator(emu, monkeypatch):
    """Same rays, no fewer cell lookups (fewer cells overflow), strictly fewer exact tests."""
    import torch
    cam, world = scenes.synthetic_analytic(n_primitives=96, seed=7, hsize=96, vsize=54)
    st = {}
    for flag in ("0", "1"):
        monkeypatch.setenv("RTC_LIGHT_GRID_TIGHT", flag)
        dr = DeviceRenderer(emu, emu.build_world(world), cam, 0, _cpu_standin=True)
        out = torch.empty(cam.vsize * cam.hsize * 3, dtype=torch.float64)
        st[flag] = dr.render_rows(3, 0, 1, cam.vsize, out, count=True, sync=True)
        st[flag]["img"] = out.clone()
    assert torch.equal(st["0"]["img"], st["1"]["img"])
    for k in ("rays_primary", "rays_shadow", "rays_reflect", "rays_refract"):
        assert st["0"][k] == st["1"][k], k
    assert st["1"]["light_grid_cells"] >= st["0"]["light_grid_cells"] > 0
    assert st["1"]["analytic_tests"] < st["0"]["analytic_tests"]
