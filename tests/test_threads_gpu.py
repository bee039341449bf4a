"""Distinct scenes from distinct host threads (include/rtc.h "Threading") on an MI355X.  The library replaces the body of a rayon
par_render, so host threads are its normal caller; every other GPU test drives its scenes from one thread.  Here every worker thread
owns its scenes and its numpy buffers and calls the C ABI through ctypes (a CDLL call releases the GIL, so the threads are inside the
library, and their kernels on the device, at the same time).  A scene used from a thread must give its SOLO frame -- the one the main
thread rendered before any worker existed -- bit for bit: pixels, hit records, hit-tree digests, explicit rays, ray counters.

Rules the file keeps: environment variables are process-global, so the main thread sets them, creates the scenes (RTC_KERNEL, RTC_WF_*
and RTC_DEVICE_BVH* are read at creation) and renders the solo references before it starts a thread, and no worker touches os.environ;
workers meet at a barrier, run ROUNDS rounds, stop at their first non-zero status and keep results and the first exception in a slot of
their own; the main thread joins with a timeout and re-raises.  A join that times out or a device error ends the whole session
(pytest.exit): nothing else may start on a device in that state.  No retries, no scene shared between threads.  The tests are ordered
from least to most concurrency.  (Times in the docstrings: one run of this file on an MI355X, set-up and solo references included.)"""
import ctypes as C
import threading
import time

import numpy as np
import pytest

import build_matrix as bm
import cases
import create_cases as cc
import ext_cases
import foreign_flattener as ff
from raytracer_challenge_amd import scenes
from raytracer_challenge_amd.backend import AdaptiveC, FilterC, RtwError, SamplingC, ShutterC
from raytracer_challenge_amd.device import DeviceRenderer, RtcCameraC, RtcStatsC
from raytracer_challenge_amd.scene import Adaptive, Camera, Filter, PointLight, Sampling, Shutter, World

pytestmark = pytest.mark.gpu
FUEL = bm.FUEL
ROUNDS = 3
JOIN_S = 120.0
RTC_ERR_DEVICE = 3
RAY_CLASSES = ("pixels", "rays_primary", "rays_shadow", "rays_reflect", "rays_refract", "rays_container")


# ---- the harness ----------------------------------------------------------------------------------------------------------------------
class Status(Exception):
    """A non-zero status of a C call made by a worker, with the calling thread's rtc_last_error()."""

    def __init__(self, code, text):
        Exception.__init__(self, "status %d: %s" % (code, text))
        self.code, self.text = code, text


def ok(lib, code):
    if code != 0:
        raise Status(code, (lib.rtc_last_error() or b"").decode())


def device_error(ex):
    """RTC_ERR_DEVICE, as a status or in the text the Python layer raises (every HIP failure names its call)."""
    if isinstance(ex, Status):
        return ex.code == RTC_ERR_DEVICE
    return isinstance(ex, RtwError) and any(w in str(ex) for w in ("hip", "guard", "HIP", "device"))


def run_threads(bodies):
    """bodies: one callable per thread, body(results).  All start together behind a barrier; returns the result lists.  The first
    exception of a worker is re-raised here, after every thread was joined."""
    gate = threading.Barrier(len(bodies))
    slots = [{"results": [], "error": None, "span": None} for _ in bodies]

    def work(body, slot):
        try:
            gate.wait(JOIN_S)
            t0 = time.perf_counter()
            body(slot["results"])
            slot["span"] = (t0, time.perf_counter())
        except BaseException as ex:  # noqa: BLE001
            slot["error"] = ex

    threads = [threading.Thread(target=work, args=(b, s), daemon=True) for b, s in zip(bodies, slots)]
    deadline = time.monotonic() + JOIN_S
    for t in threads:
        t.start()
    for t in threads:
        t.join(max(0.1, deadline - time.monotonic()))
        if t.is_alive():
            pytest.exit("test_threads_gpu: a worker thread did not come back within %d s; the device may be hung" % JOIN_S, returncode=3)
    for k, s in enumerate(slots):
        if s["error"] is not None:
            if device_error(s["error"]):
                pytest.exit("test_threads_gpu: thread %d met a device error: %s" % (k, s["error"]), returncode=3)
            raise s["error"]
    if len(slots) > 1:   # (a figure for the log, not an assertion: how long all workers were at work at once)
        first_end, last_start, last_end = min(s["span"][1] for s in slots), max(s["span"][0] for s in slots), max(s["span"][1] for s in slots)
        print("%d threads: all at work together for %.2f ms; the shortest ended after %.2f ms, the longest after %.2f ms" % (
            len(slots), 1e3 * max(0.0, first_end - last_start), 1e3 * (first_end - min(s["span"][0] for s in slots)), 1e3 * (last_end - min(s["span"][0] for s in slots))))
    return [s["results"] for s in slots]


def rounds(fn, n=ROUNDS):
    def body(out):
        for _ in range(n):
            out.append(fn())
    return body


def bits_equal(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def assert_distinct(frames, what):
    """A frame landing in the wrong thread's buffer must show: no two solo frames may hold the same bits."""
    for i in range(len(frames)):
        for j in range(i + 1, len(frames)):
            assert not bits_equal(frames[i], frames[j]), "%s: the solo frames of workers %d and %d do not differ" % (what, i, j)


def same_record(got, want, what):
    """Dicts of arrays and integers, bit for bit."""
    assert sorted(got) == sorted(want), what
    for k in want:
        if isinstance(want[k], np.ndarray):
            assert bits_equal(got[k], want[k]), "%s: %s differs from the solo result" % (what, k)
        else:
            assert got[k] == want[k], "%s: %s = %r, solo %r" % (what, k, got[k], want[k])


# ---- scenes of the build matrix, and what bm.frames_of renders of them ----------------------------------------------------------------
_rays = {}


def point_lit(world):
    """The world with every light a point light: what cases.special_rays aims at."""
    return World([l if isinstance(l, PointLight) else PointLight(l.intensity, getattr(l, "origin", None) or l.corner) for l in world.lights], world.elements)


def inputs(hip, tmp, name):
    """(camera, world, explicit rays) of a build-matrix entry at its own 48x32, or of `bumped_everything` at 24x16.  The rays the device
    refuses (RTC_ERR_NAN: the reference panics there) are left out, once per name."""
    if name == "bumped_everything":
        cam, world = ext_cases.everything_camera(24, 16), ext_cases.bumped_everything_world(True)
        aim = point_lit(world)
    else:
        entry = bm.BY_NAME[name]
        cam, world = entry.make(tmp)
        assert (cam.hsize, cam.vsize) == (48, 32)
        aim = point_lit(entry.oracle(world))
    if name not in _rays:
        rays = np.concatenate([cases.edge_rays(96), cases.special_rays(aim, 96)])
        _rays[name] = rays[bm.panic_free(hip, world, rays)]
        assert len(_rays[name]) > 96
    return cam, world, _rays[name]


def counters(hip, nw, cam):
    """The ray counters of one rtc_render with a stats pointer (bound by bm.render_with_stats)."""
    lib = hip.lib
    cc_, rc = hip.camera_c(cam), RtcCameraC()
    assert lib.rtw_make_camera(C.byref(cc_), C.byref(rc)) == 0
    n = cam.hsize * cam.vsize
    rgb, st = np.empty((n, 3)), RtcStatsC()
    ok(lib, lib.rtc_render(bm.scene_of(hip, nw), C.byref(rc), FUEL, None, 0, n, rgb.ctypes.data, None, C.byref(st)))
    d = st.as_dict()
    out = {k: d[k] for k in RAY_CLASSES + ("n_launches",)}
    out["rgb (counted)"] = rgb
    return out


class Owned:
    """One thread's scene: created, and rendered solo, on the calling (main) thread under the environment in force."""

    def __init__(self, hip, tmp, name):
        self.name, self.hip = name, hip
        self.cam, self.world, self.rays = inputs(hip, tmp, name)
        self.nw = hip.build_world(self.world)
        bm.scene_of(hip, self.nw)   # (the scene is created here: the environment is read now)
        self.want = self.everything()
        assert np.abs(self.want["rgb"]).max() > 0.1 and self.want["pixels"] == self.want["rays_primary"] == self.cam.hsize * self.cam.vsize

    def everything(self):
        """bm.frames_of -- the frame without and with counters, hit records, digests, explicit rays -- and the ray counters."""
        got = bm.frames_of(self.hip, self.nw, self.cam, self.rays)
        got.update(counters(self.hip, self.nw, self.cam))
        return got

    def check(self, results, what):
        assert len(results) == ROUNDS, what
        for r, got in enumerate(results):
            same_record(got, self.want, "%s, %s, round %d" % (what, self.name, r))
            assert bits_equal(got["rgb"], got["rgb (stats)"]) and bits_equal(got["rgb"], got["rgb (counted)"])

    def close(self):
        self.nw.close()


def render_together(hip, tmp, names, path, what):
    """One scene and one thread per name, ROUNDS rounds of everything a scene renders; every result against the solo one.  Afterwards
    every scene's sticky error state is clean and no LDS-resident launch was refused its LDS size."""
    with bm.switched("default", path):
        owned = [Owned(hip, tmp, n) for n in names]
        try:
            assert_distinct([o.want["rgb"] for o in owned], what)
            results = run_threads([rounds(o.everything) for o in owned])
            for o, res in zip(owned, results):
                o.check(res, what)
                DeviceRenderer(hip, o.nw, o.cam).check()   # rtc_scene_check: raises on a guard, a NaN or an overflow left behind
                if path == 4:
                    k = bm.kernel_info(hip, o.nw, 4, False)
                    assert k.lds_bytes == 0 or k.lds_refused == 0, "%s: the device refused %s its dynamic LDS size" % (what, o.name)
        finally:
            for o in owned:
                o.close()


# ---- 1. two scenes, two threads, synchronous calls --------------------------------------------------------------------------------------
@pytest.mark.parametrize("path", [1, 4])
def test_two_scenes_on_two_threads(hip, path, tmp_path_factory):
    """`ops12` (on path 4 the LDS-resident persistent wf_ts) beside `grid_mesh_bvh`, three rounds each of the frame without and with
    counters, hit records, digests, explicit rays and the ray counters: all equal to the solo results.  MI355X: 0.4 s on path 1 (the session's first launches), 0.1 s on path 4."""
    tmp = tmp_path_factory.mktemp("threads")
    if path == 4:
        with bm.switched("default", 4):
            o = Owned(hip, tmp, "ops12")
            k = bm.kernel_info(hip, o.nw, 4, False)
            o.close()
        assert k.lds_bytes > 0 and k.wf_ts_build == 2, "ops12 must land on the LDS build"
    render_together(hip, tmp, ["ops12", "grid_mesh_bvh"], path, "two threads, path %d" % path)


# ---- 2. one build per thread ---------------------------------------------------------------------------------------------------------
BUILDS = ["ops12", "ops12_glass_mirror", "planes7", "grid_mesh_bvh", "csg", "area_csg_real", "uv_spot_real", "bumped_everything"]


@pytest.mark.parametrize("path", [1, 4])
def test_one_kernel_build_per_thread(hip, path, tmp_path_factory):
    """Four threads (as many as hardware queues by default), then eight (more streams than queues), one scene and one kernel build each:
    rows 0, 0 without LEAN, 1, 1 with all three LDS tables, 4, 6, 11 / 10 and the BG + NP extension with wf_background.  The
    assertions of test 1; rtc_scene_check clean and no LDS size refused afterwards.  MI355X: 0.3 s on path 1, 0.5 s on path 4."""
    tmp = tmp_path_factory.mktemp("threads")
    render_together(hip, tmp, BUILDS[:4], path, "four threads, path %d" % path)
    render_together(hip, tmp, BUILDS, path, "eight threads, path %d" % path)


# ---- 3. unsynchronised frames beside synchronous ones -----------------------------------------------------------------------------------
def test_unsynchronised_frames_beside_synchronous_ones(hip, tmp_path_factory):
    """Thread A queues four rtc_render_rows_device(sync = 0) frames of `ops12` on the wavefront path -- with company alive they run on
    n_cu - spare CUs --, then rtc_scene_sync and rtc_scene_check, three times; B (`planes7`, one-kernel path) and C
    (`ops12_glass_mirror`, wavefront path) call rtc_render with a stats pointer meanwhile.  Each of A's twelve frames is its synchronous
    full-grid frame; B's and C's counters and pixels are their solo ones.  MI355X: 0.1 s."""
    import torch
    tmp = tmp_path_factory.mktemp("threads")
    with bm.switched("default", 4):
        cam, world, _ = inputs(hip, tmp, "ops12")
        nw = hip.build_world(world)
        dr = DeviceRenderer(hip, nw, cam, device=0)
        c = Owned(hip, tmp, "ops12_glass_mirror")
    with bm.switched("default", 1):
        b = Owned(hip, tmp, "planes7")
    try:
        n = cam.vsize * cam.hsize * 3
        ref_t = torch.zeros(n, dtype=torch.float64, device="cuda:0")
        outs = [torch.zeros(n, dtype=torch.float64, device="cuda:0") for _ in range(4 * ROUNDS)]
        dr.render_rows(FUEL, 0, 1, cam.vsize, ref_t, sync=True, want_stats=False)
        ref = ref_t.cpu().numpy().copy()
        torch.cuda.synchronize()   # (the buffers are zeroed on torch's stream: done before a scene's stream writes them)
        assert np.abs(ref).max() > 0.1
        k = bm.kernel_info(hip, nw, 4, False)
        g = dr.wavefront_grid(False)
        assert k.lds_bytes > 0 and g["live_scenes"] >= 3 and g["grid"] == g["n_cu"] - g["spare_cus"] < g["n_cu"], (k.lds_bytes, g)
        assert_distinct([ref.reshape(-1, 3), b.want["rgb"], c.want["rgb"]], "unsynchronised frames")

        def a_body(out):
            for r in range(ROUNDS):
                for t in outs[4 * r:4 * r + 4]:
                    dr.render_rows_async(FUEL, 0, 1, cam.vsize, t)
                ok(hip.lib, hip.lib.rtc_scene_sync(dr.scene))
                ok(hip.lib, hip.lib.rtc_scene_check(dr.scene))
                out.append(r)

        res = run_threads([a_body, rounds(lambda: counters(hip, b.nw, b.cam), 4 * ROUNDS), rounds(lambda: counters(hip, c.nw, c.cam), 4 * ROUNDS)])
        assert res[0] == list(range(ROUNDS))
        for i, t in enumerate(outs):
            got = t.cpu().numpy()
            assert got.tobytes() == ref.tobytes(), "A's frame %d: %d of %d values differ from the full-grid frame" % (i, int((got.view(np.uint64) != ref.view(np.uint64)).sum()), got.size)
        for o, got in ((b, res[1]), (c, res[2])):
            want = {key: o.want[key] for key in RAY_CLASSES + ("n_launches", "rgb (counted)")}
            assert len(got) == 4 * ROUNDS
            for i, rec in enumerate(got):
                same_record(rec, want, "%s beside unsynchronised frames, call %d" % (o.name, i))
        assert bm.kernel_info(hip, nw, 4, False).lds_refused == 0
    finally:
        nw.close()
        b.close()
        c.close()


# ---- 4. creation and destruction beside rendering ----------------------------------------------------------------------------------------
def test_creation_and_destruction_beside_rendering(hip, tmp_path_factory):
    """RTC_KERNEL unset: thread A renders `ops12_glass_mirror` eight times a round, synchronously -- the first four frames measure both paths,
    the fourth chooses -- while thread B creates, renders and destroys four scenes in a row, each round.  Two of B's are grid meshes built by the device LBVH builder on the null stream
    (RTC_DEVICE_BVH_MIN lowered beforehand; asserted); one renders a 48x32 frame twice and then a 192x128 frame twice, so that the second
    size grows d_rgb and, on its wavefront turn, the ray queues: hipFree while A renders (that scene renders four frames, not one: a
    scene's first launch of a shape takes the guessed one-kernel path, which has no queues).  Every frame is its solo frame, A's choice
    ends in (1, 4), and the device's live-scene count is back where it started.  MI355X: under 0.1 s."""
    tmp = tmp_path_factory.mktemp("threads")
    lib = hip.lib
    with bm.environment(RTC_KERNEL=None, RTC_NO_KOPS=None, RTC_KOPS_GROUPS=None, RTC_WF_LDS=None, RTC_FIRST_GUESS=None, RTC_DEVICE_BVH=None, RTC_DEVICE_BVH_MIN="64"):
        small, large = bm.camera(), bm.camera(h=192, v=128)
        jobs = [  # (label, camera(s), world, built on the device)
            ("grid 12x8", [small], bm.grid_scene(bm._grid(tmp, 12, 8))[1], 1),
            ("ops12 at two sizes", [small, small, large, large], bm.program_scene(11)[1], 0),
            ("grid 9x9 with a BVH", [small], bm.grid_scene(bm._grid(tmp, 9, 9), with_bvh=True)[1], 1),
            ("csg", [small], bm.small_world(csg=True)[1], 0),
        ]

        def life(label, cams, world, on_device, nw=None):
            """Create, render, destroy: (built on the device, frames).  nw: the world's handles, made beforehand -- the scene itself (the
            flattening, the BVHs, the uploads) is created by the first call that asks for it, here."""
            nw = nw or hip.build_world(world)
            try:
                built = lib.rtc_scene_bvh_built_on_device(bm.scene_of(hip, nw))
                return built, [hip.render(nw, cam, FUEL) for cam in cams]
            finally:
                nw.close()

        solo = [life(*j) for j in jobs]
        for j, (built, frames) in zip(jobs, solo):
            assert built == j[3], "%s: rtc_scene_bvh_built_on_device = %d" % (j[0], built)
        assert bits_equal(solo[1][1][0][0], solo[1][1][1][0]) and bits_equal(solo[1][1][2][0], solo[1][1][3][0]), "the two paths render one frame"
        a_cam, a_world = bm.program_scene(11, glass_mirror=True)
        a_solo = life("A", [a_cam], a_world, 0)[1][0]
        assert_distinct([a_solo[0]] + [f[1][0][0] for f in solo], "creation beside rendering")
        a_nw = hip.build_world(a_world)    # (A's scene anew: no launch yet, its path choice is made under contention)
        try:
            a_dr = DeviceRenderer(hip, a_nw, a_cam)
            assert a_dr.path_info()["path"] == "undecided"
            live = a_dr.wavefront_grid(False)["live_scenes"]
            # (B's handles are made beforehand: it spends its time in the library, not in Python, and more of it beside A's frames)
            ready = [(j, hip.build_world(j[2])) for _ in range(ROUNDS) for j in jobs]
            res = run_threads([rounds(lambda: hip.render(a_nw, a_cam, FUEL), 8 * ROUNDS), lambda out: out.extend(life(*j, nw=nw) for j, nw in ready)])
            assert len(res[0]) == 8 * ROUNDS and len(res[1]) == len(jobs) * ROUNDS
            for i, (rgb, hits) in enumerate(res[0]):
                assert bits_equal(rgb, a_solo[0]) and bits_equal(hits, a_solo[1]), "A's frame %d is not its solo frame" % i
            for j, (built, frames), (_, want) in zip(jobs * ROUNDS, res[1], solo * ROUNDS):
                assert built == j[3], "%s beside A: rtc_scene_bvh_built_on_device = %d" % (j[0], built)
                for i, (got, w) in enumerate(zip(frames, want)):
                    assert bits_equal(got[0], w[0]) and bits_equal(got[1], w[1]), "%s, frame %d is not its solo frame" % (j[0], i)
            assert a_dr.path_info()["path"] in ("one kernel", "wavefront"), a_dr.path_info()
            a_dr.check()
            assert a_dr.wavefront_grid(False)["live_scenes"] == live, "the live-scene count did not come back"
        finally:
            a_nw.close()


# ---- 5. a handle is not tied to its thread ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("path", [1, 4])
def test_a_handle_moves_between_threads(hip, path, tmp_path_factory):
    """Created on thread X, rendered on thread Y after X has exited, destroyed on thread Z after Y has: the solo frame.  MI355X: under 0.1 s per path."""
    tmp = tmp_path_factory.mktemp("threads")
    with bm.switched("default", path):
        solo = Owned(hip, tmp, "planes7")
        try:
            box = {}

            def create(out):
                box["nw"] = hip.build_world(solo.world)
                bm.scene_of(hip, box["nw"])
                out.append(True)

            assert run_threads([create]) == [[True]]
            got = run_threads([lambda out: out.append(bm.frames_of(hip, box["nw"], solo.cam, solo.rays))])[0][0]
            assert run_threads([lambda out: out.append(box["nw"].close())]) == [[None]]
            for k in got:
                assert bits_equal(got[k], solo.want[k]), "a handle rendered on another thread: %s differs" % k
        finally:
            solo.close()


# ---- 6. the chunked entry points -----------------------------------------------------------------------------------------------------------
def chunked_jobs(hip):
    """[(name, call)]: one chunked entry point each on scenes of its own; call() makes the C call into fresh numpy buffers and returns
    {pixels, rays_primary, ...}.  Everything a call needs is made here, on the calling thread."""
    from test_filter_gpu import MITCHELL_CASE
    sl = al = fl = hl = hip.lib
    keep, jobs = [], []

    def scene(world):
        nw = hip.build_world(world)
        keep.append(nw)
        return bm.scene_of(hip, nw)

    def sampled():
        cam, world = scenes.chapter11_glass_air_bubble(37, 19)
        s, rc, sp, n = scene(world), hip._rtc_camera(cam), SamplingC.of(Sampling(side=3, jitter=True, seed=5)), 37 * 19

        def call():
            rgb, st = np.full((n, 3), np.nan), RtcStatsC()
            ok(sl, sl.rtc_render_sampled(s, C.byref(rc), C.byref(sp), 5, None, 0, n, rgb.ctypes.data, C.byref(st)))
            return {"rgb": rgb, "rays_primary": int(st.rays_primary)}
        return call

    def filtered(name, size, sampling, flt):
        cam, world = getattr(scenes, name)(*size)
        s, rc, sp, fc, n = scene(world), hip._rtc_camera(cam), SamplingC.of(sampling), FilterC.of(flt), size[0] * size[1]

        def call():
            rgb, st = np.full((n, 3), np.nan), RtcStatsC()
            ok(fl, fl.rtc_render_filtered(s, C.byref(rc), C.byref(sp), C.byref(fc), 5, 0, size[1], rgb.ctypes.data, C.byref(st)))
            return {"rgb": rgb, "rays_primary": int(st.rays_primary)}
        return call

    def adaptive():
        cam, world = scenes.texture_showcase(24, 16)   # (test_adaptive_gpu.KINDS: flat regions and edges at this threshold)
        ad = AdaptiveC.of(Adaptive(Sampling(), Sampling(side=3, jitter=True, seed=6), 0.3, 8))
        s, rc, n = scene(world), hip._rtc_camera(cam), 24 * 16

        def call():
            rgb, mask, n_ref, st = np.full((n, 3), np.nan), np.full(n, 7, dtype=np.uint8), C.c_uint64(1 << 63), RtcStatsC()
            ok(al, al.rtc_render_adaptive(s, C.byref(rc), C.byref(ad), 5, rgb.ctypes.data, mask.ctypes.data, C.byref(n_ref), C.byref(st)))
            return {"rgb": rgb, "mask": mask, "n_refined": int(n_ref.value), "rays_primary": int(st.rays_primary)}
        return call

    def shutter():
        poses = scenes.motion_showcase(37, 19, 3)
        K, n = len(poses), 37 * 19
        ss, cams = (C.c_void_p * K)(*[scene(w) for _, w in poses]), (RtcCameraC * K)()
        for p, (cam, _) in enumerate(poses):
            cams[p] = hip._rtc_camera(cam)
        sp, sh = SamplingC.of(Sampling(side=3, jitter=True, seed=29)), ShutterC.of(Shutter())

        def call():
            rgb, st = np.full((n, 3), np.nan), RtcStatsC()
            ok(hl, hl.rtc_render_shutter(ss, cams, K, C.byref(sh), C.byref(sp), 5, None, 0, n, rgb.ctypes.data, C.byref(st)))
            return {"rgb": rgb, "rays_primary": int(st.rays_primary)}
        return call

    jobs.append(("rtc_render_sampled", sampled()))
    jobs.append(("rtc_render_filtered, Mitchell", filtered(*MITCHELL_CASE)))
    jobs.append(("rtc_render_filtered, box 0.5", filtered("cover", (24, 16), Sampling(side=2, jitter=True, seed=7), Filter.box(0.5))))
    jobs.append(("rtc_render_adaptive", adaptive()))
    jobs.append(("rtc_render_shutter", shutter()))
    return jobs, keep


@pytest.mark.parametrize("path", ["1", "4"])
def test_chunked_entry_points_on_a_thread_each(hip, path):
    """rtc_render_sampled, rtc_render_filtered (the Mitchell gather and the half-pixel box, which is the sampled mean), rtc_render_adaptive
    and rtc_render_shutter over three poses, one thread each on scenes no other thread uses, RTC_SAMPLED_MAX_RAYS=3000 so that every call
    runs several chunks (the scratch buffers, the scan and the dealing of five calls in flight at once).  Pixels, masks, n_refined and
    rays_primary equal the solo results.  MI355X: 0.1 s on path 1, 0.3 s on path 4."""
    with bm.environment(RTC_KERNEL=path, RTC_SAMPLED_MAX_RAYS="3000", RTC_FILTER_LDS=None, RTC_NO_KOPS=None, RTC_KOPS_GROUPS=None, RTC_WF_LDS=None):
        jobs, keep = chunked_jobs(hip)
        try:
            solo = [call() for _, call in jobs]
            for (name, _), s in zip(jobs, solo):
                assert np.isfinite(s["rgb"]).all() and s["rgb"].max() > 0.1 and s["rays_primary"] >= len(s["rgb"]), name
            ad = solo[3]
            assert 0 < ad["n_refined"] < len(ad["mask"]) and int(ad["mask"].sum()) == ad["n_refined"] and set(np.unique(ad["mask"]).tolist()) == {0, 1}
            assert ad["rays_primary"] == len(ad["mask"]) + 9 * ad["n_refined"]
            assert_distinct([s["rgb"] for s in solo], "chunked entry points")
            res = run_threads([rounds(call) for _, call in jobs])
            for (name, _), got, want in zip(jobs, res, solo):
                assert len(got) == ROUNDS
                for r, rec in enumerate(got):
                    same_record(rec, want, "%s on a thread of its own, path %s, round %d" % (name, path, r))
        finally:
            for nw in keep:
                nw.close()


# ---- 7. rtc_multi beside plain scenes ----------------------------------------------------------------------------------------------------
def test_rtc_multi_beside_plain_scenes(hip, tmp_path_factory):
    """One thread renders rtc_render_multi and rtc_render_multi_rgb8 over three replicas on device 0 in bands of 5 rows (41x23: rows no
    multiple of the band); two threads render scenes of their own.  The multi frame is the one-device frame of the same descriptor, as
    in test_cabi_desc.test_hip_render_multi_random_partitions.  MI355X: 0.1 s."""
    tmp = tmp_path_factory.mktemp("threads")
    lib = hip.lib
    vp = C.c_void_p
    with bm.switched("default", 4):
        others = [Owned(hip, tmp, "ops12"), Owned(hip, tmp, "csg")]
        cam0, world = cases.SMALL_CASES["nested_glass"]()
        cam = Camera.new(41, 23, cam0.field_of_view, cam0.transform_matrix)
        flat = ff.flatten(world)
        desc, multi, scene = flat.desc(), vp(), vp()
        cc_, rc = hip.camera_c(cam), RtcCameraC()
        assert lib.rtw_make_camera(C.byref(cc_), C.byref(rc)) == 0
        n = 41 * 23
        try:
            assert cc.create(lib, "rtc_multi_create", desc, multi, devices=(0, 0, 0)) == 0, lib.rtc_last_error()
            assert cc.create(lib, "rtc_scene_create", desc, scene) == 0, lib.rtc_last_error()
            assert lib.rtc_multi_set_band_rows(multi, 5) == 0
            one = np.empty((n, 3))
            ok(lib, lib.rtc_render(scene, C.byref(rc), 4, None, 0, n, one.ctypes.data, None, None))

            def multi_call():
                rgb, rgb8 = np.full((n, 3), np.nan), np.full(n * 3, 7, dtype=np.uint8)
                ok(lib, lib.rtc_render_multi(multi, C.byref(rc), 4, rgb.ctypes.data, None))
                ok(lib, lib.rtc_render_multi_rgb8(multi, C.byref(rc), 4, rgb8.ctypes.data, None))
                return {"rgb": rgb, "rgb8": rgb8}

            solo = multi_call()
            assert bits_equal(solo["rgb"], one), "rtc_render_multi is not the one-device frame"
            assert solo["rgb8"].max() > 7
            assert_distinct([one] + [o.want["rgb"] for o in others], "rtc_multi beside plain scenes")
            res = run_threads([rounds(multi_call)] + [rounds(o.everything) for o in others])
            for r, rec in enumerate(res[0]):
                same_record(rec, solo, "rtc_render_multi beside two scenes, round %d" % r)
                assert bits_equal(rec["rgb"], one)
            for o, got in zip(others, res[1:]):
                o.check(got, "beside rtc_render_multi")
        finally:
            if multi:
                lib.rtc_multi_destroy(multi)
            if scene:
                lib.rtc_scene_destroy(scene)
            for o in others:
                o.close()


# ---- 8. errors belong to the caller ---------------------------------------------------------------------------------------------------------
def test_errors_belong_to_the_calling_thread(hip, tmp_path_factory):
    """Thread A asks for refusals that never reach a kernel -- fuel 17, an empty and an out-of-image row range of rtc_render_filtered --
    3 000 times in turn, and reads its own rtc_last_error() text after each; thread B is refused once (a sampling of side 0), then renders successfully
    twelve times: rtc_last_error() returns B's text after every frame, never A's, and the frames are B's solo frames.  (The CPU twin,
    test_threads_cpu.py, fails with `thread_local` taken off the error strings.)  MI355X: under 0.1 s."""
    tmp = tmp_path_factory.mktemp("threads")
    lib = hip.lib
    with bm.switched("default", 1):
        a, b = Owned(hip, tmp, "csg"), Owned(hip, tmp, "planes7")
    try:
        FUEL_TEXT = b"fuel exceeds RTC_MAX_FUEL (16)"
        ROWS_TEXT = b"filtered: the row range is empty or leaves the image"
        SIDE_TEXT = b"sampling: side must be >= 1"
        A_CALLS = 1000 * ROUNDS   # (a refusal takes microseconds: this many last as long as B's frames do)
        n = a.cam.hsize * a.cam.vsize
        a_scene, b_scene = bm.scene_of(hip, a.nw), bm.scene_of(hip, b.nw)
        a_cam, b_cam = hip._rtc_camera(a.cam), hip._rtc_camera(b.cam)
        sp, zero, box = SamplingC.of(Sampling(side=2)), SamplingC.of(Sampling(side=1)), FilterC.of(Filter.tent(1.5))
        zero.side = 0
        b_solo = hip.render(b.nw, b.cam, FUEL)
        hip.render(a.nw, a.cam, FUEL)   # (A's output buffers exist: its refusals allocate nothing)

        def a_body(out):
            rgb = np.empty((n, 3))
            rc_cam = C.pointer(a_cam)
            for i in range(A_CALLS):
                if i % 3 == 0:
                    code, want = lib.rtc_render(a_scene, rc_cam, 17, None, 0, n, rgb.ctypes.data, None, None), (2, FUEL_TEXT)
                elif i % 3 == 1:
                    code, want = lib.rtc_render_filtered(a_scene, C.byref(a_cam), C.byref(sp), C.byref(box), FUEL, 0, 0, rgb.ctypes.data, None), (1, ROWS_TEXT)
                else:
                    code, want = lib.rtc_render_filtered(a_scene, C.byref(a_cam), C.byref(sp), C.byref(box), FUEL, a.cam.vsize, 1, rgb.ctypes.data, None), (1, ROWS_TEXT)
                text = lib.rtc_last_error()
                assert code == want[0] and text.startswith(want[1]), "thread A, call %d: status %d, rtc_last_error() = %r; its own refusal reads %r" % (i, code, text, want[1])
                out.append(i)

        def b_body(out):
            rgb = np.empty((n, 3))
            code = lib.rtc_render_sampled(b_scene, C.byref(b_cam), C.byref(zero), FUEL, None, 0, n, rgb.ctypes.data, None)
            assert code == 1 and lib.rtc_last_error() == SIDE_TEXT, (code, lib.rtc_last_error())
            for i in range(4 * ROUNDS):
                frame = hip.render(b.nw, b.cam, FUEL)
                text = lib.rtc_last_error()
                assert text == SIDE_TEXT, "thread B after frame %d: rtc_last_error() = %r, its refusal read %r" % (i, text, SIDE_TEXT)
                out.append(frame)

        res = run_threads([a_body, b_body])
        assert len(res[0]) == A_CALLS and len(res[1]) == 4 * ROUNDS
        for i, (rgb, hits) in enumerate(res[1]):
            assert bits_equal(rgb, b_solo[0]) and bits_equal(hits, b_solo[1]), "B's frame %d is not its solo frame" % i
        DeviceRenderer(hip, a.nw, a.cam).check()
        DeviceRenderer(hip, b.nw, b.cam).check()
    finally:
        a.close()
        b.close()
