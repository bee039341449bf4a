#!/usr/bin/env python3
"""Cost of the shutter (include/rtc.h rtc_shutter) on config 2's scene at fuel 5: the 1920x1080 frame, 4x4 jittered samples per pixel,
through rtc_render_shutter with K = 1, 4 and 16 EQUAL poses (one scene handle and one camera K times, RTC_SHUTTER_HASHED) beside
rtc_render_sampled with the same sampling -- the same pixels, bit for bit, so the difference is what the dealing, the per-pose launches
and the scattered rays cost.  Both calls hand host pixels back, so the figure is wall clock around the call, warmed; ROUNDS rounds that
alternate over all configurations in one process, so every figure has a run-to-run spread (min / median / max over the rounds).  On each
pinned device path and with the library choosing (a shutter's runs take the scene's first guess, rtc_render_sampled measures).

Alongside: one frame with counters per K (RTC_SAMPLED_TIMING=1: the events around a chunk's parts, read back from stderr): the share
of the dealing kernels, the generators and the resolve in kernel_ms.

usage: shutter_probe.py [FRAMES [ROUNDS]]     (GPU)
       shutter_probe.py --resource-usage      (no GPU: the compiler's figures for the rtc_shutter_* kernels)"""
import ctypes as C
import json
import os
import re
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
CSRC = os.path.join(ROOT, "raytracer_challenge_amd", "csrc")
POSES = (1, 4, 16)


def resource_usage():
    out = subprocess.run(["make", "-s", "-C", CSRC, "resource-usage", "VARIANTS="], check=True, stdout=subprocess.PIPE, text=True).stdout
    for line in out.splitlines():
        if "rtc_shutter_" in line:
            print("  " + "  ".join(line.split("\t")))


def main(frames, rounds):
    import numpy as np
    import raytracer_challenge_amd as rt
    from raytracer_challenge_amd import scenes
    from raytracer_challenge_amd.backend import SamplingC, ShutterC
    from raytracer_challenge_amd.device import RtcCameraC, RtcStatsC
    from raytracer_challenge_amd.scene import Sampling, Shutter

    cam, world = scenes.synthetic_analytic(n_primitives=512, seed=12345, cones=False, grouped=False, hsize=1920, vsize=1080)
    be = rt.hip_backend()
    lib = be.lib
    vp = C.c_void_p
    rc_cam = be._rtc_camera(cam)
    cams = (RtcCameraC * max(POSES))(*[rc_cam] * max(POSES))
    sp, sh = SamplingC.of(Sampling(side=4, jitter=True, seed=1)), ShutterC.of(Shutter(hashed=True))
    n = 1920 * 1080
    rgb, ref = np.empty((n, 3)), np.empty((n, 3))

    # one scene per path setting (RTC_KERNEL is read when a scene is created)
    scene_of, worlds = {}, []
    for path in ("1", "4", "auto"):
        if path == "auto":
            os.environ.pop("RTC_KERNEL", None)
        else:
            os.environ["RTC_KERNEL"] = path
        nw = be.build_world(world)
        worlds.append(nw)
        scene_of[path] = lib.rtw_world_scene(nw.handle, 0)
        assert scene_of[path], be._err()
    os.environ.pop("RTC_KERNEL", None)

    def frame(scene, K, out, stats=None):
        st = None if stats is None else C.byref(stats)
        if K == 0:
            code = lib.rtc_render_sampled(scene, C.byref(rc_cam), C.byref(sp), 5, None, 0, n, out.ctypes.data, st)
        else:
            code = lib.rtc_render_shutter((vp * K)(*[scene] * K), cams, K, C.byref(sh), C.byref(sp), 5, None, 0, n, out.ctypes.data, st)
        assert code == 0, lib.rtc_last_error()

    def timed(scene, K):
        t0 = time.perf_counter()
        for _ in range(frames):
            frame(scene, K, rgb)
        return (time.perf_counter() - t0) * 1e3 / frames

    def label(K):
        return "rtc_render_sampled" if K == 0 else "rtc_render_shutter K=%d" % K
    configs = (0,) + POSES
    # warm-up: code loading, queues, buffers; with the library choosing, the four synchronous launches of rtc_render_sampled's measurement
    same = {}
    for path, scene in scene_of.items():
        for _ in range(4):
            frame(scene, 0, ref)
        for K in POSES:
            frame(scene, K, rgb)
            frame(scene, K, rgb)
            same["%s | path %s" % (label(K), path)] = bool(np.array_equal(rgb.view(np.uint64), ref.view(np.uint64)))
    print("bit-identical to rtc_render_sampled: %s" % ("all" if all(same.values()) else same), flush=True)
    results = {}
    for r in range(rounds):
        for K in configs:
            for path, scene in scene_of.items():
                results.setdefault((label(K), path), []).append(timed(scene, K))
    print("ms per frame (wall clock, host pixels), min / median / max over %d rounds of %d frames:" % (rounds, frames))
    table = {}
    for (lb, path), v in results.items():
        table["%s | path %s" % (lb, path)] = {"min": min(v), "median": statistics.median(v), "max": max(v)}
        base = statistics.median(results[(label(0), path)])
        print("  %-26s path %-4s  %8.3f / %8.3f / %8.3f   x %.3f of rtc_render_sampled" % (lb, path, min(v), statistics.median(v), max(v), statistics.median(v) / base), flush=True)

    # the parts: one frame with counters per K and path, the chunks' parts read back from stderr
    parts = {}
    os.environ["RTC_SAMPLED_TIMING"] = "1"
    pat = re.compile(r"\[rtc-shutter\] chunk of \d+ rays: dealing ([\d.]+) ms \((\d+) kernels\), generators ([\d.]+) ms, traces ([\d.]+) ms, resolve ([\d.]+) ms")
    for path, scene in scene_of.items():
        for K in POSES:
            st = RtcStatsC()
            sys.stderr.flush()
            with tempfile.TemporaryFile(mode="w+") as tmp:
                saved = os.dup(2)
                os.dup2(tmp.fileno(), 2)
                try:
                    frame(scene, K, rgb, stats=st)
                finally:
                    os.dup2(saved, 2)
                    os.close(saved)
                tmp.seek(0)
                rows = [tuple(float(x) for x in m.groups()) for m in pat.finditer(tmp.read())]
            deal, gen, trace, res = (sum(r[i] for r in rows) for i in (0, 2, 3, 4))
            parts["K=%d | path %s" % (K, path)] = {"kernel_ms": st.kernel_ms, "n_launches": st.n_launches, "chunks": len(rows), "dealing_ms": deal, "generators_ms": gen,
                                                  "traces_ms": trace, "resolve_ms": res}
            print("  with counters, K=%-2d path %-4s: kernel_ms %8.3f in %d launches, %d chunks: dealing %.3f ms (%.2f %%), generators %.3f ms, traces %.3f ms, resolve %.3f ms"
                  % (K, path, st.kernel_ms, st.n_launches, len(rows), deal, 100.0 * deal / st.kernel_ms, gen, trace, res), flush=True)
    os.environ.pop("RTC_SAMPLED_TIMING")
    print(json.dumps({"frames": frames, "rounds": rounds, "ms": table, "bit_identical": same, "parts": parts}))


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "--resource-usage":
        resource_usage()
    else:
        main(int(sys.argv[1]) if len(sys.argv) > 1 else 3, int(sys.argv[2]) if len(sys.argv) > 2 else 5)
