#!/usr/bin/env python3
"""Cost of adaptive sampling (include/rtc.h rtc_adaptive) on config 2's scene at fuel 5: the 1920x1080 frame rendered plain
(rtc_render), fully 4x4 jittered (rtc_render_sampled) and adaptively (rtc_render_adaptive: base side 1, fine 4x4 jittered) at the
thresholds 0.05, 0.1 and 0.3, on each pinned device path.  All three are host-pixel calls without counters, timed alike: device time
between two stream markers around K calls, so each figure holds the frame's copy to the host and, for the adaptive frame, the idle
time of its one read-back.  Warmed; ROUNDS rounds that alternate over all configurations in one process, so every figure has a
run-to-run spread (min / median / max over the rounds).

Alongside, per threshold and path: the refined share, from one call with counters (RTC_SAMPLED_TIMING=1: the library's events) the
detect + compact time and the sum of the chunks' scatter-resolve times, and from the counters the rays a primary ray's tree holds over
the refined pixels against the whole frame's (what the refined pixels cost beyond their share).

The bar (printed at the end, per path and threshold): the adaptive frame may cost the same run's plain frame, plus the refined share times
the same run's full 4x4 frame, plus the time one read and one write of the frame (24 B per pixel) and of the list (8 B per refined
pixel) need at the HBM peak (8.0 TB/s), plus the run-to-run spread (max - min) of the two reference figures.

usage: adaptive_probe.py [K [ROUNDS]]     (GPU)
       adaptive_probe.py --resource-usage  (no GPU: the compiler's figures for the kernels of rtc_adaptive.hip)"""
import ctypes as C
import json
import os
import re
import statistics
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
CSRC = os.path.join(ROOT, "raytracer_challenge_amd", "csrc")
HBM_PEAK = 8.0e12   # bytes / s
KERNELS = ("rtc_contrast_flags", "rtc_scan_tiles", "rtc_scan_add_base", "rtc_contrast_scatter", "rtc_resolve_samples_scatter")


def resource_usage():
    out = subprocess.run(["make", "-s", "-C", CSRC, "resource-usage", "VARIANTS="], check=True, stdout=subprocess.PIPE, text=True).stdout
    for line in out.splitlines():
        if any(k in line for k in KERNELS):
            print("  " + "  ".join(line.split("\t")))


class stderr_to_file:
    """The library's debug lines go to the C stderr: collect them for the duration of a call."""

    def __enter__(self):
        sys.stderr.flush()
        self.tmp = tempfile.TemporaryFile(mode="w+b")
        self.saved = os.dup(2)
        os.dup2(self.tmp.fileno(), 2)
        return self

    def __exit__(self, *exc):
        os.dup2(self.saved, 2)
        os.close(self.saved)
        self.tmp.seek(0)
        self.text = self.tmp.read().decode(errors="replace")
        self.tmp.close()
        return False


def main(k, rounds):
    import numpy as np
    import raytracer_challenge_amd as rt
    from raytracer_challenge_amd import scenes
    from raytracer_challenge_amd.backend import AdaptiveC, SamplingC
    from raytracer_challenge_amd.device import RtcStatsC
    from raytracer_challenge_amd.scene import Adaptive, Sampling

    cam, world = scenes.synthetic_analytic(n_primitives=512, seed=12345, cones=False, grouped=False, hsize=1920, vsize=1080)
    be = rt.hip_backend()
    lib = be.lib
    vp = C.c_void_p

    rc_cam = be._rtc_camera(cam)
    n = 1920 * 1080
    rgb = np.zeros((n, 3))   # (written once here: every call finds the pages present)
    fine = Sampling(side=4, jitter=True, seed=1)
    fine_c = SamplingC.of(fine)
    thresholds = (0.05, 0.1, 0.3)
    rules = {t: AdaptiveC.of(Adaptive(Sampling(), fine, t)) for t in thresholds}

    # one scene per pinned path (RTC_KERNEL is read when a scene is created)
    scene_of, worlds = {}, []
    for path in ("1", "4"):
        os.environ["RTC_KERNEL"] = path
        nw = be.build_world(world)
        worlds.append(nw)
        scene_of[path] = lib.rtw_world_scene(nw.handle, 0)
        assert scene_of[path], be._err()
    os.environ.pop("RTC_KERNEL", None)

    def call(scene, cfg, stats=None, n_refined=None):
        if cfg == "plain":
            return lib.rtc_render(scene, rc_cam, 5, None, 0, n, rgb.ctypes.data, None, stats)
        if cfg == "full 4x4":
            return lib.rtc_render_sampled(scene, rc_cam, C.byref(fine_c), 5, None, 0, n, rgb.ctypes.data, stats)
        return lib.rtc_render_adaptive(scene, rc_cam, C.byref(rules[cfg]), 5, rgb.ctypes.data, None, n_refined, stats)

    def timed(scene, cfg, frames):
        assert lib.rtc_scene_record(scene, 0) == 0
        for _ in range(frames):
            assert call(scene, cfg) == 0, lib.rtc_last_error()
        assert lib.rtc_scene_record(scene, 1) == 0 and lib.rtc_scene_wait(scene, 1) == 0
        ms = C.c_double()
        assert lib.rtc_scene_elapsed_ms(scene, 0, 1, C.byref(ms)) == 0
        return ms.value / frames

    configs = ["plain", "full 4x4"] + list(thresholds)

    def label(cfg):
        return cfg if isinstance(cfg, str) else "adaptive %.2f" % cfg
    # warm-up (code loading, queues, buffers), the refined shares, and the library's own events for the parts
    share, parts = {}, {}

    def all_rays(st):
        return st.rays_primary + st.rays_shadow + st.rays_reflect + st.rays_refract
    for path, scene in scene_of.items():
        for cfg in configs:
            for _ in range(2):
                assert call(scene, cfg) == 0, lib.rtc_last_error()
        st_full = RtcStatsC()
        assert call(scene, "full 4x4", C.byref(st_full)) == 0, lib.rtc_last_error()
        st_plain = RtcStatsC()
        assert call(scene, "plain", C.byref(st_plain)) == 0, lib.rtc_last_error()
        tree_full = all_rays(st_full) / st_full.rays_primary   # rays of the average primary ray's tree, over the whole frame
        for t in thresholds:
            st, nr = RtcStatsC(), C.c_uint64(0)
            os.environ["RTC_SAMPLED_TIMING"] = "1"
            with stderr_to_file() as err:
                code = call(scene, t, C.byref(st), C.byref(nr))
            os.environ.pop("RTC_SAMPLED_TIMING")
            assert code == 0, lib.rtc_last_error()
            detect = [float(x) for x in re.findall(r"\[rtc-adaptive\] detect \+ compact ([0-9.]+) ms", err.text)]
            resolve = [float(x) for x in re.findall(r"resolve ([0-9.]+) ms", err.text)]
            assert len(detect) == 1 and st.rays_primary == n + 16 * nr.value, (err.text, st.rays_primary, nr.value)
            share[(t, path)] = nr.value / n
            tree_refined = (all_rays(st) - all_rays(st_plain)) / (16.0 * nr.value)   # the same over the refined pixels' sixteen samples
            print("%-14s path %s: rays per primary ray: %.2f over the refined pixels, %.2f over the full 4x4 frame" % (label(t), path, tree_refined, tree_full), flush=True)
            parts["%s | path %s" % (label(t), path)] = {"n_refined": nr.value, "share": nr.value / n, "detect_compact_ms": detect[0], "scatter_resolve_ms": sum(resolve),
                                                       "rays_per_primary_refined": tree_refined, "rays_per_primary_full_frame": tree_full,
                                                       "chunks": len(resolve), "kernel_ms_with_counters": st.kernel_ms, "n_launches": st.n_launches}
            print("%-14s path %s: %8d of %d pixels refined (%5.2f %%); detect + compact %.3f ms; scatter resolve %.3f ms over %d chunks" %
                  (label(t), path, nr.value, n, 100.0 * nr.value / n, detect[0], sum(resolve), len(resolve)), flush=True)
    results = {}
    for r in range(rounds):
        for cfg in configs:
            for path, scene in scene_of.items():
                results.setdefault((label(cfg), path), []).append(timed(scene, cfg, k))
    print("ms per frame (host pixels), min / median / max over %d rounds of %d frames:" % (rounds, k))
    table = {}
    for (lb, path), v in results.items():
        table["%s | path %s" % (lb, path)] = {"min": min(v), "median": statistics.median(v), "max": max(v)}
        print("  %-14s path %s  %8.3f / %8.3f / %8.3f" % (lb, path, min(v), statistics.median(v), max(v)), flush=True)

    # the bar
    bar = {}
    for path in scene_of:
        plain, full = table["plain | path %s" % path], table["full 4x4 | path %s" % path]
        spread = (plain["max"] - plain["min"]) + (full["max"] - full["min"])
        for t in thresholds:
            s = share[(t, path)]
            traffic_ms = 2.0 * (n * 24 + s * n * 8) / HBM_PEAK * 1e3
            allowed = plain["median"] + s * full["median"] + traffic_ms + spread
            got = table["%s | path %s" % (label(t), path)]["median"]
            bar["%s | path %s" % (label(t), path)] = {"measured_ms": got, "bar_ms": allowed, "plain_ms": plain["median"], "share_times_full_ms": s * full["median"],
                                                     "traffic_ms": traffic_ms, "spread_ms": spread, "within": got <= allowed}
            print("bar, path %s, %-14s: measured %.3f ms; bar %.3f ms = plain %.3f + %.4f x full %.3f + traffic %.3f + spread %.3f: %s"
                  % (path, label(t), got, allowed, plain["median"], s, full["median"], traffic_ms, spread, "within" if got <= allowed else "OVER"))
    print(json.dumps({"k": k, "rounds": rounds, "ms": table, "parts": parts, "bar": bar}))


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "--resource-usage":
        resource_usage()
    else:
        main(int(sys.argv[1]) if len(sys.argv) > 1 else 3, int(sys.argv[2]) if len(sys.argv) > 2 else 5)
