"""Every build of the ray kernels pinned to a scene, and the builds held to one answer (on an MI355X).

The ray kernels exist in several builds per row of the variant table (DESIGN.md "Kernel builds"); a chain of host decisions picks the
build that renders a scene.  tests/build_matrix.py restates those decisions and lists small scenes constructed to land on each build.
Here the library is asked which build it would launch (rtc_scene_kernel_info) and held to the restatement (the ledger); every scene is
rendered under every build it can be switched to -- both paths, RTC_NO_KOPS, RTC_KOPS_GROUPS=0, RTC_WF_LDS=0, with and without
counters -- and all frames, hit records, digests and explicit rays must be the same bits; one of them is compared with the oracle."""
import ctypes as C
import math
import time

import numpy as np
import pytest

import build_matrix as bm
import foreign_flattener as ff
from build_matrix import Entry, Facts
from raytracer_challenge_amd import scenes

pytestmark = pytest.mark.gpu


# ---- entries whose size is computed on the device ---------------------------------------------------------------------------------------
def lds_report(hip, world):
    """(hook's LDS bytes, the restated figure from the hook's own counts) of the wavefront path's traversal kernel."""
    with bm.switched("default", 4):
        nw = hip.build_world(world)
        k = bm.kernel_info(hip, nw, 4, False)
        nw.close()
    table = bm.lds_table_bytes(k.n_bvh_nodes, k.n_recs, k.n_mesh_tris, k.has_recs, k.has_mesh)
    return k, bm.lds_bytes(k.variant, True, table, k.bvh_stack)


@pytest.fixture(scope="module")
def lds_pair(hip, tmp_path_factory):
    """Two grid meshes one triangle apart, the smaller LDS-resident and the larger not: bisection over the number of faces written of
    one grid; every probe's report must equal the restated rtc_lds_table_bytes + RTC_LDS_BLOCK * bvh_stack * 4 <= 158 KiB."""
    tmp = tmp_path_factory.mktemp("lds_pair")

    def probe(n_faces):
        _, world = bm.grid_scene(bm._grid(tmp, 40, 40, n_faces))
        k, want = lds_report(hip, world)
        assert k.lds_bytes == want and k.n_mesh_tris == n_faces, (n_faces, k.lds_bytes, want, k.n_mesh_tris)
        return k.lds_bytes > 0

    lo, hi = 64, 2 * 39 * 39
    assert probe(lo) and not probe(hi)
    while hi - lo > 1:
        mid = (lo + hi) // 2
        if probe(mid):
            lo = mid
        else:
            hi = mid
    under = Entry("lds_just_under", lambda t: bm.grid_scene(bm._grid(tmp, 40, 40, lo)), Facts(1, True, all_plain=True, lds=True), (1, 1), "the largest mesh whose tables fit LDS")
    over = Entry("lds_just_over", lambda t: bm.grid_scene(bm._grid(tmp, 40, 40, hi)), Facts(1, True, all_plain=True, lds=False), (1, 1), "one triangle more: tables in memory")
    return under, over


def device_bytes(hip, world):
    nw = hip.build_world(world)
    b = int(hip.lib.rtc_scene_device_bytes(bm.scene_of(hip, nw)))
    nw.close()
    return b


@pytest.fixture(scope="module")
def big_entry(hip, tmp_path_factory):
    """The smallest square heightfield (config 5's scene at 48x32) whose device tables exceed 32 MiB: the grid side from the bytes per
    triangle of two small probes, then stepped until the library calls the scene big and the grid one vertex smaller not."""
    tmp = tmp_path_factory.mktemp("big")

    def world(n):
        return scenes.synthetic_mesh(str(tmp / ("hf%d.obj" % n)), nx=n, nz=n, hsize=48, vsize=32)

    b0, b1 = device_bytes(hip, world(20)[1]), device_bytes(hip, world(40)[1])
    per_tri = (b1 - b0) / (2 * 39 * 39 - 2 * 19 * 19)
    n = int(math.sqrt(bm.BIG_SCENE / per_tri / 2)) + 1
    for _ in range(16):
        if device_bytes(hip, world(n)[1]) > bm.BIG_SCENE:
            break
        n += 1
    while device_bytes(hip, world(n - 1)[1]) > bm.BIG_SCENE:
        n -= 1
    assert device_bytes(hip, world(n)[1]) > bm.BIG_SCENE >= device_bytes(hip, world(n - 1)[1])
    print("3-wave entry: %d x %d grid, %d triangles, %.1f MiB" % (n, n, 2 * (n - 1) ** 2, device_bytes(hip, world(n)[1]) / 2 ** 20))
    return Entry("big_mesh", lambda t: world(n), Facts(1, True, no_glass_mirror=False, big=True), (1, 1), "3-waves-per-SIMD build of rows 1 and 2")


# ---- 1. the ledger ------------------------------------------------------------------------------------------------------------------------
def test_ledger(hip, lds_pair, big_entry, tmp_path):
    """Every (row, kernel, build) of the restatement is reported for at least one entry under one of its switches; every entry reports
    exactly the build the table names, under every switch; the switches that change nothing are the ones the table predicts."""
    entries = bm.TABLE + list(lds_pair) + [big_entry]
    ledger, skipped = set(), []
    for e in entries:
        _, world = e.make(tmp_path)
        for switch in bm.SWITCHES:
            changed = bm.check_hook(hip, e, world, switch, False, ledger)
            if switch != "default" and not changed:
                skipped.append((e.name, switch))
    want = bm.all_builds()
    assert want <= ledger, "no entry of the table runs %s" % sorted(want - ledger, key=str)
    assert ledger <= want, "the library reports builds the restatement does not know: %s" % sorted(ledger - want, key=str)
    assert sorted(skipped) == bm.predicted_skips(entries, False)


def test_lds_layout_edges(hip, lds_pair, tmp_path):
    """The LDS-resident entries sit on the layout's edges: a triangle table that is no multiple of 16 B, node and record tables that are
    no multiple of the copying block, with and without records, with and without a mesh; the hook's size is the restated one."""
    seen = set()
    for e in [x for x in bm.TABLE if x.facts.lds] + [lds_pair[0]]:
        k, want = lds_report(hip, e.make(tmp_path)[1])
        assert k.lds_bytes == want > 0 and k.variant in (0, 1, 5), (e.name, k.lds_bytes, want, k.variant)
        with bm.switched("default", 4):
            nw = hip.build_world(e.make(tmp_path)[1])
            assert int(hip.lib.rtc_scene_wavefront_lds_bytes(bm.scene_of(hip, nw))) == want   # (the older query agrees)
            nw.close()
        seen.add((bool(k.has_recs), bool(k.has_mesh), k.n_bvh_nodes > 0))
        if e.name.startswith("grid_mesh"):
            assert (76 * k.n_mesh_tris) % 16 != 0, (e.name, k.n_mesh_tris)
        if k.n_bvh_nodes:
            assert (8 * k.n_bvh_nodes) % bm.LDS_BLOCK != 0, (e.name, k.n_bvh_nodes)
        if k.has_recs:
            assert (8 * k.n_recs) % bm.LDS_BLOCK != 0, (e.name, k.n_recs)
    assert {(False, True, True), (True, False, True), (True, True, True)} <= seen, seen   # mesh only / analytic BVH only / both
    k, want = lds_report(hip, lds_pair[1].make(tmp_path)[1])
    assert k.lds_bytes == want == 0
    assert k.n_mesh_tris == lds_report(hip, lds_pair[0].make(tmp_path)[1])[0].n_mesh_tris + 1


# ---- 2 + 3. one answer per scene, tied to the oracle ------------------------------------------------------------------------------------
@pytest.mark.parametrize("entry", bm.TABLE, ids=repr)
def test_one_answer(hip, orc, entry, tmp_path):
    skipped = bm.one_answer(hip, orc, entry, tmp_path, False)
    assert sorted(skipped) == bm.predicted_skips([entry], False)


@pytest.mark.parametrize("which", [0, 1], ids=["just_under", "just_over"])
def test_one_answer_at_the_lds_limit(hip, orc, lds_pair, which, tmp_path):
    skipped = bm.one_answer(hip, orc, lds_pair[which], tmp_path, False)
    assert sorted(skipped) == bm.predicted_skips([lds_pair[which]], False)


def test_one_answer_big_mesh(hip, orc, big_entry, tmp_path):
    """The one heavy case: the smallest heightfield above 32 MiB, so that the one-kernel path takes its 3-waves-per-SIMD build (rows 1
    and, under RTC_NO_KOPS, 2).  The oracle has no accelerator and needs about 0.2 s per ray tree on this mesh (57 s for 256 pixels on a
    CPU), so it renders a fixed list of 48 pixels and 16 of the explicit rays; the full 48x32 frame and all 2 048 explicit rays -- the
    panicking ones found by the device's own refusal -- are compared build against build: 3wave, count, RTC_NO_KOPS, the wavefront path.
    Measured on an MI355X: the time this test prints (DESIGN.md quotes it); every other case here takes under 0.4 s."""
    t0 = time.time()
    skipped = bm.one_answer(hip, orc, big_entry, tmp_path, False, oracle_pixels=np.arange(7, 48 * 32, 32, dtype=np.uint64), oracle_rays=16)
    assert sorted(skipped) == bm.predicted_skips([big_entry], False)
    print("big_mesh: %.1f s" % (time.time() - t0))


# ---- 4. several devices -----------------------------------------------------------------------------------------------------------------
def test_lds_resident_scene_on_several_devices(hip, tmp_path):
    """rtc_render_multi of an LDS-resident scene over 2 and over min(4, n) devices: the one-device frame, bit for bit.  The dynamic-LDS
    attribute of the traversal kernel is raised once per device (a bitmask in launch_wf_ts_lds): a device other than 0 must get its own."""
    n_dev = int(hip.lib.rtc_device_count())
    if n_dev < 2:
        pytest.skip("needs two devices")
    lib = hip.lib
    vp = C.c_void_p
    entry = bm.BY_NAME["grid_mesh_bvh"]
    cam, world = entry.make(tmp_path)
    k, want = lds_report(hip, world)
    assert k.lds_bytes == want > 0
    with bm.switched("default", 4):
        one = hip.render(hip.build_world(world), cam, bm.FUEL)[0]
        flat = ff.flatten(world)   # (owns the arrays the descriptor points to)
        desc, rc = flat.desc(), ff.make_camera(cam)
        for n in sorted({2, min(4, n_dev)}):
            m, devs = vp(), (C.c_int * n)(*range(n))
            assert lib.rtc_multi_create(C.byref(desc), devs, n, C.byref(m)) == 0, lib.rtc_last_error()
            rgb = np.full((cam.hsize * cam.vsize, 3), np.nan)
            assert lib.rtc_render_multi(m, C.byref(rc), bm.FUEL, rgb.ctypes.data, None) == 0, lib.rtc_last_error()
            lib.rtc_multi_destroy(m)
            assert np.array_equal(rgb.view(np.uint64), one.view(np.uint64)), "%d devices" % n
        for d in range(min(4, n_dev)):   # no device fell back to the memory build: a scene of its own there reports the LDS build, unrefused
            nw = hip.build_world(world)
            k = bm.kernel_info(hip, nw, 4, False, device=d)
            assert k.lds_bytes == want and k.lds_refused == 0, (d, k.lds_bytes, k.lds_refused)
            nw.close()
