"""Spare CUs of the LDS-resident wavefront traversal build (include/rtc.h rtc_scene_wavefront_ts_grid, RTC_WF_SPARE_CUS) on
an MI355X.  An unsynchronised launch of a scene that has company on its device runs wf_ts on n_cu - k blocks; the kernel hands out its
chunks from cursors, so every grid must render the bits of the full one.  Scene: tests/build_matrix.py `ops12` at 48x32 and fuel 5, which
lands on the LDS build (asserted); RTC_KERNEL=4 pins the wavefront path."""
import ctypes as C
import gc

import numpy as np
import pytest

import build_matrix as bm

pytestmark = pytest.mark.gpu
FUEL = bm.FUEL


def renderer(hip, world, cam, **env):
    """(world handle, DeviceRenderer) of a fresh scene created under RTC_KERNEL=4 and `env` (None: unset)."""
    from raytracer_challenge_amd.device import DeviceRenderer
    kw = {"RTC_KERNEL": "4", "RTC_WF_LDS": None, "RTC_WF_SPARE_CUS": None, "RTC_NO_KOPS": None, "RTC_KOPS_GROUPS": None}
    kw.update(env)
    with bm.environment(**kw):
        nw = hip.build_world(world)
        return nw, DeviceRenderer(hip, nw, cam, device=0)   # (the scene is created here: the environment is read now)


def info_of(hip, nw):
    k = bm.KernelInfo()
    assert hip.lib.rtc_scene_kernel_info(bm.scene_of(hip, nw), 4, 0, C.byref(k)) == 0, hip.lib.rtc_last_error()
    return k


def frame_sync(dr, cam, count=False):
    """(pixels, stats) of one synchronous launch."""
    import torch
    out = torch.zeros(cam.vsize * cam.hsize * 3, dtype=torch.float64, device="cuda:0")
    st = dr.render_rows(FUEL, 0, 1, cam.vsize, out, count=count, sync=True, want_stats=count)
    return out.cpu().numpy().copy(), st


def frame_async(dr, cam):
    """The pixels of one unsynchronised row launch followed by a wait; the sticky error state must be clean."""
    import torch
    out = torch.zeros(cam.vsize * cam.hsize * 3, dtype=torch.float64, device="cuda:0")
    dr.render_rows_async(FUEL, 0, 1, cam.vsize, out)
    dr.sync()
    dr.check()   # raises on a guard, a NaN or an overflow left behind
    return out.cpu().numpy().copy()


@pytest.fixture(scope="module")
def setup(hip, tmp_path_factory):
    """The scene, and its full-grid frame: rendered synchronously by a scene of its own, once, shared by the tests."""
    import torch
    cam, world = bm.BY_NAME["ops12"].make(tmp_path_factory.mktemp("spare"))
    assert (cam.hsize, cam.vsize) == (48, 32)
    n_cu = torch.cuda.get_device_properties(0).multi_processor_count
    nw, dr = renderer(hip, world, cam)
    k = info_of(hip, nw)
    assert k.lds_bytes > 0 and k.wf_ts_build == 2, "ops12 must land on the LDS build"
    ref, _ = frame_sync(dr, cam)
    assert info_of(hip, nw).lds_refused == 0, "the device refused the dynamic LDS size"
    assert dr.wavefront_grid(True)["n_cu"] == n_cu
    nw.close()
    assert np.abs(ref).max() > 0.1
    return cam, world, n_cu, ref


def spare_values(n_cu):
    return [(0, n_cu), (8, n_cu - 8), (n_cu - 8, 8), (n_cu - 3, 3), (n_cu - 1, 1), (n_cu + 5, 1)]


def test_every_grid_renders_the_full_grid_frame(hip, setup):
    """Two scenes alive; unsynchronised launches under RTC_WF_SPARE_CUS = 0, 8, n_cu - 8 (8 blocks), n_cu - 3 (3 blocks: fewer cursor
    residues than 8), n_cu - 1 (one block) and n_cu + 5 (clamped to one block): each frame equals the synchronous, full-grid one bit for
    bit, and no error state is left behind."""
    cam, world, n_cu, ref = setup
    company_nw, company = renderer(hip, world, cam)
    try:
        for k, grid in spare_values(n_cu):
            nw, dr = renderer(hip, world, cam, RTC_WF_SPARE_CUS=str(k))
            try:
                info = info_of(hip, nw)
                assert info.lds_bytes > 0 and info.lds_refused == 0
                g = dr.wavefront_grid(False)
                assert g["live_scenes"] >= 2 and g["grid"] == grid, (k, g)
                got = frame_async(dr, cam)
                assert got.tobytes() == ref.tobytes(), "RTC_WF_SPARE_CUS=%d (a grid of %d blocks): %d of %d values differ from the full-grid frame" % (
                    k, grid, int((got.view(np.uint64) != ref.view(np.uint64)).sum()), got.size)
                assert info_of(hip, nw).lds_refused == 0
                # the company's stream at work meanwhile changes nothing either: both scenes queue a frame, then both are waited for
                import torch
                a = torch.zeros(cam.vsize * cam.hsize * 3, dtype=torch.float64, device="cuda:0")
                b = torch.zeros_like(a)
                company.render_rows_async(FUEL, 0, 1, cam.vsize, a)
                dr.render_rows_async(FUEL, 0, 1, cam.vsize, b)
                company.sync(); dr.sync()
                company.check(); dr.check()
                assert a.cpu().numpy().tobytes() == ref.tobytes() and b.cpu().numpy().tobytes() == ref.tobytes(), k
            finally:
                nw.close()
    finally:
        company_nw.close()


def test_query_reports_the_grid_a_launch_takes(hip, setup):
    """n_cu - k for the unsynchronised launch of a scene that has company, the full grid for a synchronous launch, and the full grid
    again once the scene is the only one alive."""
    cam, world, n_cu, ref = setup
    gc.collect()
    nw, dr = renderer(hip, world, cam, RTC_WF_SPARE_CUS="8")
    try:
        before = dr.wavefront_grid(False)
        others = before["live_scenes"] - 1   # (scenes other tests of this process still hold: none when this file runs alone)
        assert before["n_cu"] == n_cu and before["spare_cus"] == 8
        assert before["grid"] == (n_cu - 8 if others else n_cu), before
        company_nw, company = renderer(hip, world, cam)
        with_company = dr.wavefront_grid(False)
        assert with_company["live_scenes"] == others + 2
        assert with_company["grid"] == n_cu - 8, with_company
        assert dr.wavefront_grid(True)["grid"] == n_cu, "a synchronous launch takes every CU"
        assert company.wavefront_grid(True)["grid"] == n_cu
        assert company.wavefront_grid(False)["grid"] == n_cu - company.wavefront_grid(False)["spare_cus"]   # (created without the variable: the built-in number)
        company_nw.close()   # destroys the other scene
        alone = dr.wavefront_grid(False)
        assert alone["live_scenes"] == others + 1
        assert alone["grid"] == (n_cu - 8 if others else n_cu), alone
        assert dr.wavefront_grid(True)["grid"] == n_cu
        assert frame_async(dr, cam).tobytes() == ref.tobytes()
    finally:
        nw.close()
    # clamping, as the scene keeps it
    for k, want in (("-4", 0), ("0", 0), (str(n_cu - 1), n_cu - 1), (str(n_cu + 5), n_cu - 1)):
        nw, dr = renderer(hip, world, cam, RTC_WF_SPARE_CUS=k)
        try:
            assert dr.wavefront_grid(False)["spare_cus"] == want, k
        finally:
            nw.close()


def test_memory_build_ignores_the_switch(hip, setup):
    """RTC_WF_LDS=0: the one-wave blocks of the memory build are spread over every CU by the dispatcher, so the switch leaves their grid
    alone: the same report and the same bits for every value."""
    cam, world, n_cu, ref = setup
    company_nw, company = renderer(hip, world, cam, RTC_WF_LDS="0")
    try:
        reports = []
        for k, _ in spare_values(n_cu):
            nw, dr = renderer(hip, world, cam, RTC_WF_LDS="0", RTC_WF_SPARE_CUS=str(k))
            try:
                info = info_of(hip, nw)
                assert info.lds_bytes == 0 and info.wf_ts_build == 0
                reports.append((dr.wavefront_grid(False)["grid"], dr.wavefront_grid(True)["grid"]))
                assert frame_async(dr, cam).tobytes() == ref.tobytes(), k
                assert frame_sync(dr, cam)[0].tobytes() == ref.tobytes(), k
            finally:
                nw.close()
        assert len(set(reports)) == 1 and reports[0][0] == reports[0][1] and reports[0][0] >= n_cu, reports
    finally:
        company_nw.close()


def test_counting_launches_sum_to_the_same_counters(hip, setup):
    """One counting launch of a scene created with 0 spare CUs and one of a scene created with n_cu - 3, company alive: equal ray counters
    (and the frame's bits).  A launch that hands its counters back has a stats pointer, so the host waits for it and BOTH take the full
    grid: this pins that the switch does not reach counting launches.  The counting build (RTC_WF_TS_LDS_COUNT) on a small grid is
    exercised by the launch in front of it: counters on, no stats pointer, unsynchronised -- 3 blocks at k = n_cu - 3 -- whose frame must
    be the reference's bits (no call reads the counters back after an unsynchronised launch)."""
    import torch
    cam, world, n_cu, ref = setup
    company_nw, company = renderer(hip, world, cam)
    try:
        stats = []
        for k in (0, n_cu - 3):
            nw, dr = renderer(hip, world, cam, RTC_WF_SPARE_CUS=str(k))
            try:
                assert dr.wavefront_grid(False)["grid"] == n_cu - k and dr.wavefront_grid(True)["grid"] == n_cu
                out = torch.zeros(cam.vsize * cam.hsize * 3, dtype=torch.float64, device="cuda:0")
                dr._rc(dr._bands(None, FUEL, 1, 0, 1, cam.vsize, out, None, True, False), "rtc_render_bands_device")   # count = 1, stats = NULL, sync = 0
                dr.sync()
                dr.check()
                assert out.cpu().numpy().tobytes() == ref.tobytes(), "counting build, unsynchronised, RTC_WF_SPARE_CUS=%d" % k
                k4 = bm.KernelInfo()
                assert hip.lib.rtc_scene_kernel_info(bm.scene_of(hip, nw), 4, 1, C.byref(k4)) == 0
                assert k4.wf_ts_build == 3 and k4.lds_refused == 0   # RTC_WF_TS_LDS_COUNT
                got, st = frame_sync(dr, cam, count=True)
                assert got.tobytes() == ref.tobytes(), k
                stats.append({key: st[key] for key in ("pixels", "rays_primary", "rays_shadow", "rays_reflect", "rays_refract", "rays_container", "unique_rays")})
            finally:
                nw.close()
        assert stats[0] == stats[1], stats
        assert stats[0]["rays_primary"] == cam.hsize * cam.vsize and stats[0]["rays_reflect"] > 0 and stats[0]["rays_shadow"] > 0
    finally:
        company_nw.close()
