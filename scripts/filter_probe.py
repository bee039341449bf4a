#!/usr/bin/env python3
"""Cost of the pixel reconstruction filters (include/rtc.h rtc_filter) on config 2's scene at fuel 5: the 1920x1080 frame with 4x4
jittered samples as HOST pixels (wall clock around the call), through rtc_render_sampled -- the reference figure: code the filters do
not touch -- and through rtc_render_filtered with BOX 0.5, TENT 1.5 and MITCHELL 2.0, on each pinned device path.  ROUNDS rounds
alternate over all configurations in one process, so every figure has a run-to-run spread (min / median / max over the rounds).

Alongside, per filter and path, one synchronous frame with stats under RTC_SAMPLED_TIMING=1: the rows actually traced (halo rows are
traced by both neighbouring chunks), the gather kernel's own time summed over the chunks (the library's events), the branch and tile
it took; and the same frame with RTC_FILTER_LDS=0, the memory branch.

The bar for a filtered frame (printed at the end): the same run's sampled frame times (rows traced / rows of the frame), plus one read
of the samples (24 B each) and one write of the frame at the HBM peak (8.0 TB/s), plus the run-to-run spread of the sampled figure.

usage: filter_probe.py [ROUNDS] [--out FILE]      (GPU; FILE defaults to profiles/filter_probe.txt)
       filter_probe.py --resource-usage            (no GPU: the compiler's figures for rtc_resolve_filtered)"""
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
HBM_PEAK = 8.0e12   # bytes / s


def resource_usage():
    out = subprocess.run(["make", "-s", "-C", CSRC, "resource-usage", "VARIANTS="], check=True, stdout=subprocess.PIPE, text=True).stdout
    for line in out.splitlines():
        if "rtc_resolve_filtered" in line:
            print("  " + "  ".join(line.split("\t")))


def main(rounds, out_path):
    import numpy as np
    import raytracer_challenge_amd as rt
    from raytracer_challenge_amd import scenes
    from raytracer_challenge_amd.backend import FilterC, SamplingC
    from raytracer_challenge_amd.device import RtcStatsC
    from raytracer_challenge_amd.scene import Filter, Sampling

    lines = []

    def say(text):
        print(text, flush=True)
        lines.append(text)

    W, H, SIDE = 1920, 1080, 4
    cam, world = scenes.synthetic_analytic(n_primitives=512, seed=12345, cones=False, grouped=False, hsize=W, vsize=H)
    be = rt.hip_backend()
    lib = be.lib
    vp = C.c_void_p
    rc = be._rtc_camera(cam)
    sp = SamplingC.of(Sampling(side=SIDE, jitter=True, seed=1))
    n = W * H
    rgb = np.empty((n, 3))

    scene_of, worlds = {}, []
    for path in ("1", "4"):   # RTC_KERNEL is read when a scene is created
        os.environ["RTC_KERNEL"] = path
        nw = be.build_world(world)
        worlds.append(nw)
        scene_of[path] = lib.rtw_world_scene(nw.handle, 0)
        assert scene_of[path], be._err()
    os.environ.pop("RTC_KERNEL", None)

    filters = {"box 0.5": Filter.box(0.5), "tent 1.5": Filter.tent(1.5), "mitchell 2.0": Filter.mitchell(2.0)}
    configs = ["sampled"] + list(filters)

    def frame(scene, cfg, stats=None):
        st = None if stats is None else C.byref(stats)
        if cfg == "sampled":
            code = lib.rtc_render_sampled(scene, rc, C.byref(sp), 5, None, 0, n, rgb.ctypes.data, st)
        else:
            fl = FilterC.of(filters[cfg])
            code = lib.rtc_render_filtered(scene, rc, C.byref(sp), C.byref(fl), 5, 0, H, rgb.ctypes.data, st)
        assert code == 0, lib.rtc_last_error()

    def with_stderr(fn):
        """fn() with the process's stderr (the library writes its timing lines there) collected."""
        sys.stderr.flush()
        with tempfile.TemporaryFile(mode="w+b") as tmp:
            saved = os.dup(2)
            os.dup2(tmp.fileno(), 2)
            try:
                fn()
            finally:
                os.dup2(saved, 2)
                os.close(saved)
            tmp.seek(0)
            return tmp.read().decode(errors="replace")

    for path, scene in scene_of.items():   # warm-up: code loading, queues, buffers, the destination's pages
        for cfg in configs:
            for _ in range(2):
                frame(scene, cfg)
    ms = {}
    for _ in range(rounds):
        for cfg in configs:
            for path, scene in scene_of.items():
                t0 = time.perf_counter()
                frame(scene, cfg)
                ms.setdefault((cfg, path), []).append((time.perf_counter() - t0) * 1e3)
    say("config 2, %dx%d, %dx%d jittered samples, fuel 5, host pixels: ms per frame (wall clock), min / median / max over %d rounds" % (W, H, SIDE, SIDE, rounds))
    table = {}
    for (cfg, path), v in ms.items():
        table["%s | path %s" % (cfg, path)] = {"min": min(v), "median": statistics.median(v), "max": max(v)}
        say("  %-14s path %s  %9.3f / %9.3f / %9.3f" % (cfg, path, min(v), statistics.median(v), max(v)))

    # the parts: one synchronous frame with stats per filter, path and branch
    parts = {}
    os.environ["RTC_SAMPLED_TIMING"] = "1"
    for lds in ("default", "0"):
        if lds == "0":
            os.environ["RTC_FILTER_LDS"] = "0"
        for cfg in filters:
            for path, scene in scene_of.items():
                st = RtcStatsC()
                err = with_stderr(lambda: frame(scene, cfg, st))
                chunks = re.findall(r"\[rtc-filtered\] chunk of (\d+) rays for (\d+) rows: generator ([\d.]+) ms, traces ([\d.]+) ms, filter ([\d.]+) ms \((\w+), tile (\d+x\d+), (\d+) B", err)
                rows_traced = st.rays_primary / (W * SIDE * SIDE)
                p = {"chunks": len(chunks), "rows_traced": rows_traced, "kernel_ms": st.kernel_ms, "generator_ms": sum(float(c[2]) for c in chunks),
                     "traces_ms": sum(float(c[3]) for c in chunks), "filter_ms": sum(float(c[4]) for c in chunks),
                     "branch": sorted({c[5] for c in chunks}), "tile": sorted({c[6] for c in chunks}), "lds_bytes": sorted({int(c[7]) for c in chunks})}
                parts["%s | path %s | RTC_FILTER_LDS %s" % (cfg, path, lds)] = p
                say("  parts (counting kernels), %-12s path %s, RTC_FILTER_LDS %-7s: %d chunks, %.0f rows traced for %d; generator %.3f ms, traces %.3f ms, filter kernel %.3f ms"
                    " (%s, tile %s, %s B of LDS)" % (cfg, path, lds, p["chunks"], rows_traced, H, p["generator_ms"], p["traces_ms"], p["filter_ms"], "/".join(p["branch"]),
                                                     "/".join(p["tile"]), "/".join(str(b) for b in p["lds_bytes"])))
    os.environ.pop("RTC_FILTER_LDS", None)
    os.environ.pop("RTC_SAMPLED_TIMING")

    # the bar
    traffic_ms = (n * SIDE * SIDE * 24 + n * 24) / HBM_PEAK * 1e3
    bar = {}
    for path in scene_of:
        ref = table["sampled | path %s" % path]
        spread = ref["max"] - ref["min"]
        for cfg in filters:
            rows = parts["%s | path %s | RTC_FILTER_LDS default" % (cfg, path)]["rows_traced"]
            allowed = ref["median"] * rows / H + traffic_ms + spread
            got = table["%s | path %s" % (cfg, path)]["median"]
            bar["%s | path %s" % (cfg, path)] = {"ms": got, "allowed_ms": allowed, "sampled_ms": ref["median"], "rows_traced": rows, "traffic_ms": traffic_ms,
                                                 "spread_ms": spread, "within": got <= allowed}
            say("bar, %-12s path %s: %.3f ms; allowed %.3f ms = sampled %.3f x %.0f / %d rows + traffic at the HBM peak %.3f + sampled spread %.3f: %s"
                % (cfg, path, got, allowed, ref["median"], rows, H, traffic_ms, spread, "within" if got <= allowed else "OVER"))
    say(json.dumps({"rounds": rounds, "ms": table, "parts": parts, "bar": bar}))
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    args = sys.argv[1:]
    if args and args[0] == "--resource-usage":
        resource_usage()
    else:
        out = os.path.join(ROOT, "profiles", "filter_probe.txt")
        if "--out" in args:
            i = args.index("--out")
            out = args[i + 1]
            del args[i:i + 2]
        main(int(args[0]) if args else 7, out)
