#!/usr/bin/env python3
"""Cost of a scene background (include/rtc.h rtc_background) on config 2 and config 3 at 1920x1080, fuel 5, as HOST pixels (wall clock
around rtc_render), on each pinned device path.  ROUNDS rounds alternate over all frames in one process, so every figure has a run-to-run
spread (min / median / max over the rounds).  Both configs stand between two walls: they are opened up (the walls taken away) so that the
part of the frame above the horizon, and many reflected rays, hit nothing.  The frames, per config:
  closed    the config as it is (no ray of the camera misses)
  open      without the two walls, no background: the misses are black
  sky       the same with scenes.sky_showcase's gradient sky
For sky against open the frame time, the share of camera rays that miss and rtc_stats.kernel_ms stand side by side; the hit records and
the ray counters of the two must be equal (a background traces no ray), which is checked here too.

    background_probe.py [ROUNDS] [--out FILE]          (GPU; FILE defaults to profiles/background_probe.txt)
    background_probe.py --trace-frames N               render N frames of config 2's sky frame on the wavefront path and nothing else: the
                                                       program to run under `rocprofv3 --kernel-trace --stats`
    background_probe.py --trace-summary DIR [--out FILE]   wf_background's time per level from that run's *_kernel_trace.csv, appended to FILE
    background_probe.py --build-times BEFORE_S AFTER_S [--out FILE]   append the library's build times (measured by the caller with `time make`)"""
import csv
import ctypes as C
import glob
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
W, H, FUEL = 1920, 1080, 5


def worlds():
    from raytracer_challenge_amd import scenes
    from raytracer_challenge_amd.scene import World
    sky = scenes.sky_showcase(8, 8)[1].background
    out = {}
    for name, (cam, world) in (("config2", scenes.synthetic_analytic(n_primitives=512, seed=12345, cones=False, grouped=False, hsize=W, vsize=H)),
                               ("config3", scenes.chapter15_teapot("teapot_low.obj", W, H))):
        opened = [world.elements[0]] + world.elements[3:]          # the floor stays, the two walls go
        out[name] = (cam, {"closed": world, "open": World(world.lights, opened), "sky": World(world.lights, opened, sky)})
    return out


def bound(be):
    lib = be.lib
    vp = C.c_void_p
    return lib


def main(rounds, out_path):
    import numpy as np
    import raytracer_challenge_amd as rt
    from raytracer_challenge_amd.backend import HIT_DTYPE
    from raytracer_challenge_amd.device import RtcStatsC

    lines = []

    def say(text):
        print(text, flush=True)
        lines.append(text)

    be = rt.hip_backend()
    lib = bound(be)
    n = W * H
    rgb, hits = np.empty((n, 3)), np.empty(n, dtype=HIT_DTYPE)
    scene_of, cams, keep = {}, {}, []
    for config, (cam, frames) in worlds().items():
        rc = be._rtc_camera(cam)
        cams[config] = rc
        for path in ("1", "4"):   # RTC_KERNEL is read when a scene is created
            os.environ["RTC_KERNEL"] = path
            for name, w in frames.items():
                nw = be.build_world(w)
                keep.append(nw)
                scene_of[(config, name, path)] = lib.rtw_world_scene(nw.handle, 0)
                assert scene_of[(config, name, path)], be._err()
    os.environ.pop("RTC_KERNEL", None)

    def frame(key, stats=None, want_hits=False):
        code = lib.rtc_render(scene_of[key], cams[key[0]], FUEL, None, 0, n, rgb.ctypes.data, hits.ctypes.data if want_hits else None, None if stats is None else C.byref(stats))
        assert code == 0, lib.rtc_last_error()

    counted, pixels, records = {}, {}, {}
    for key in scene_of:   # warm-up (code loading, queues, buffers, the destination's pages), then one counted frame
        for _ in range(2):
            frame(key)
        st = RtcStatsC()
        frame(key, st, True)
        counted[key] = {k: int(getattr(st, k)) for k in ("rays_primary", "rays_shadow", "rays_reflect", "rays_refract", "n_launches")}
        counted[key]["kernel_ms"] = float(st.kernel_ms)
        counted[key]["miss_share"] = float((hits["prim"] < 0).mean())
        pixels[key], records[key] = rgb.copy(), hits.copy()
    ms = {}
    for _ in range(rounds):
        for key in scene_of:
            t0 = time.perf_counter()
            frame(key)
            ms.setdefault(key, []).append((time.perf_counter() - t0) * 1e3)

    say("%dx%d, fuel %d, host pixels: ms per frame (wall clock), min / median / max over %d rounds; kernel_ms, camera rays that miss and launches of one counted frame" % (
        W, H, FUEL, rounds))
    table = {}
    for key, v in ms.items():
        c = counted[key]
        table[" | ".join(key)] = {"min": min(v), "median": statistics.median(v), "max": max(v), **c}
        say("  %-8s %-6s path %s  %9.3f / %9.3f / %9.3f   kernel_ms %8.3f   misses %5.1f %%   launches %2d" % (
            key[0], key[1], key[2], min(v), statistics.median(v), max(v), c["kernel_ms"], 100.0 * c["miss_share"], c["n_launches"]))
    checks = {}
    for config in ("config2", "config3"):
        for path in ("1", "4"):
            a, b = (config, "open", path), (config, "sky", path)
            same = records[a].tobytes() == records[b].tobytes() and all(counted[a][k] == counted[b][k] for k in ("rays_primary", "rays_shadow", "rays_reflect", "rays_refract"))
            checks["%s path %s: sky has open's hits and ray counters" % (config, path)] = bool(same)
            say("  %s path %s: sky has open's hit records and ray counters: %s" % (config, path, same))
            x, r = table[" | ".join(b)], table[" | ".join(a)]
            say("  %s path %s: sky %.3f ms against open %.3f ms (%.3f x; open's spread %.3f ms); kernel_ms %.3f against %.3f" % (
                config, path, x["median"], r["median"], x["median"] / r["median"], r["max"] - r["min"], x["kernel_ms"], r["kernel_ms"]))
        for name in ("closed", "open", "sky"):
            same = bool(np.array_equal(pixels[(config, name, "1")].view(np.uint64), pixels[(config, name, "4")].view(np.uint64)))
            checks["%s %s: path 1 == path 4" % (config, name)] = same
            say("  %s %-6s: both paths give the same bits: %s" % (config, name, same))
    say(json.dumps({"rounds": rounds, "ms": table, "checks": checks}))
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        f.write("\n".join(lines) + "\n")


def trace_frames(count):
    import numpy as np
    import raytracer_challenge_amd as rt
    os.environ["RTC_KERNEL"] = "4"
    be = rt.hip_backend()
    lib = bound(be)
    cam, frames = worlds()["config2"]
    rc = be._rtc_camera(cam)
    nw = be.build_world(frames["sky"])
    scene = lib.rtw_world_scene(nw.handle, 0)
    assert scene, be._err()
    rgb = np.empty((W * H, 3))
    for _ in range(count):
        assert lib.rtc_render(scene, rc, FUEL, None, 0, W * H, rgb.ctypes.data, None, None) == 0, lib.rtc_last_error()


def trace_summary(directory, out_path):
    """wf_background is launched once per level, level 0 first: launch k of a frame (in start order) is level k % (FUEL + 1)."""
    rows = []
    for path in glob.glob(os.path.join(directory, "**", "*kernel_trace.csv"), recursive=True):
        with open(path, newline="") as f:
            rows += [r for r in csv.DictReader(f)]
    name_key = next(k for k in rows[0] if k.lower() in ("kernel_name", "kernelname", "name"))
    start_key = next(k for k in rows[0] if k.lower() in ("start_timestamp", "begin_ns", "start"))
    end_key = next(k for k in rows[0] if k.lower() in ("end_timestamp", "end_ns", "end"))
    rows.sort(key=lambda r: int(r[start_key]))
    total = {}
    for r in rows:
        kernel = r[name_key].split("(")[0]
        kernel = "wf_ts" if "wf_ts" in kernel else "wf_shade" if "wf_shade" in kernel else "wf_background" if "wf_background" in kernel else "wf_gather" if "wf_gather" in kernel else kernel
        total.setdefault(kernel, []).append((int(r[end_key]) - int(r[start_key])) / 1e3)
    bg = total.get("wf_background", [])
    frames = len(bg) // (FUEL + 1)
    lines = ["rocprofv3 --kernel-trace --stats, config 2 opened up with the gradient sky, wavefront path, %d frames: device time in us (per level: without the first two frames)" % frames]
    for kernel in ("wf_ts", "wf_shade", "wf_background", "wf_gather"):
        v = total.get(kernel, [])
        if v:
            lines.append("  %-14s %5d launches, %10.1f us per frame (mean over all frames)" % (kernel, len(v), sum(v) / max(1, frames)))
    for level in range(FUEL + 1):
        v = bg[level::FUEL + 1][2:] or bg[level::FUEL + 1]
        lines.append("  wf_background level %d: min / median / max %8.1f / %8.1f / %8.1f us" % (level, min(v), statistics.median(v), max(v)))
    print("\n".join(lines))
    with open(out_path, "a") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    args = sys.argv[1:]
    out = os.path.join(ROOT, "profiles", "background_probe.txt")
    if "--out" in args:
        i = args.index("--out")
        out = args[i + 1]
        del args[i:i + 2]
    if args and args[0] == "--trace-frames":
        trace_frames(int(args[1]))
    elif args and args[0] == "--trace-summary":
        trace_summary(args[1], out)
    elif args and args[0] == "--build-times":
        line = "library build (make -j8, 8 CPUs, no GPU): %.1f s before, %.1f s after (the background: 7 more objects, 12 more instantiations of rtc_trace_kernel)" % (
            float(args[1]), float(args[2]))
        print(line)
        with open(out, "a") as f:
            f.write(line + "\n")
    else:
        main(int(args[0]) if args else 7, out)
