#!/usr/bin/env python3
"""Cost of light cones (include/rtc.h rtc_light_cone) on config 2's scene at 1920x1080, fuel 5, as HOST pixels (wall clock around
rtc_render), on each pinned device path.  ROUNDS rounds alternate over all frames in one process, so every figure has a run-to-run
spread (min / median / max over the rounds).  The frames:
  a        the scene's two lights written as 1x1 area lights at their origins: the area kernels (no cone code) -- the reference frame
  b        the same lights with an open cone, cos_inner = cos_outer = -1: the SPOT kernels, every sample lit
  c        the same lights with a cone aimed at the scene's centre that lights about a quarter of its 40 x 40 footprint
  d0 / d   the lights as 4x4 jittered area lights of 10 x 10 units, without a cone / with c's cone
The bar for b (printed at the end): a's median plus a's spread over the rounds.  For c and d the frame time and rtc_stats.rays_shadow
stand beside the cone-less frame's (a, d0).

usage: spot_probe.py [ROUNDS] [--out FILE]      (GPU; FILE defaults to profiles/spot_probe.txt)"""
import ctypes as C
import json
import math
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main(rounds, out_path):
    import numpy as np
    import raytracer_challenge_amd as rt
    from raytracer_challenge_amd import scenes
    from raytracer_challenge_amd.device import RtcStatsC
    from raytracer_challenge_amd.scene import AreaLight, Cone, Vector, World

    lines = []

    def say(text):
        print(text, flush=True)
        lines.append(text)

    W, H, FUEL = 1920, 1080, 5
    cam, world = scenes.synthetic_analytic(n_primitives=512, seed=12345, cones=False, grouped=False, hsize=W, vsize=H)
    zero = Vector.vector(0.0, 0.0, 0.0)

    def lights(steps, size, cone):
        out = []
        for l in world.lights:
            o = l.origin
            axis = Vector.vector(-o[0], -o[1], -o[2])   # towards the scene's centre
            k = None if cone is None else Cone(axis, *cone)
            if steps == 1:
                out.append(AreaLight(l.intensity, o, zero, 1, zero, 1, cone=k))
            else:
                out.append(AreaLight(l.intensity, Vector.point(o[0] - 0.5 * size, o[1], o[2] - 0.5 * size), Vector.vector(size, 0.0, 0.0), steps,
                                     Vector.vector(0.0, 0.0, size), steps, jitter=True, cone=k))
        return World(out, world.elements)

    dist = math.sqrt(sum(x * x for x in world.lights[0].origin[:3]))
    quarter = (math.atan(9.0 / dist), math.atan(13.5 / dist))   # a pool of radius ~ 11 at the centre: about a quarter of 40 x 40
    frames = {"a": lights(1, 0.0, None), "b": lights(1, 0.0, (math.pi, math.pi)), "c": lights(1, 0.0, quarter),
              "d0": lights(4, 10.0, None), "d": lights(4, 10.0, quarter)}

    be = rt.hip_backend()
    lib = be.lib
    vp = C.c_void_p
    rc = be._rtc_camera(cam)
    n = W * H
    rgb = np.empty((n, 3))

    scene_of, keep = {}, []
    for path in ("1", "4"):   # RTC_KERNEL is read when a scene is created
        os.environ["RTC_KERNEL"] = path
        for name, w in frames.items():
            nw = be.build_world(w)
            keep.append(nw)
            scene_of[(name, path)] = lib.rtw_world_scene(nw.handle, 0)
            assert scene_of[(name, path)], be._err()
    os.environ.pop("RTC_KERNEL", None)

    def frame(key, stats=None):
        code = lib.rtc_render(scene_of[key], rc, FUEL, None, 0, n, rgb.ctypes.data, None, None if stats is None else C.byref(stats))
        assert code == 0, lib.rtc_last_error()

    shadow, pixels = {}, {}
    for key in scene_of:   # warm-up (code loading, queues, buffers, the destination's pages), then one counted frame
        for _ in range(2):
            frame(key)
        st = RtcStatsC()
        frame(key, st)
        shadow[key] = int(st.rays_shadow)
        pixels[key] = rgb.copy()
    ms = {}
    for _ in range(rounds):
        for key in scene_of:
            t0 = time.perf_counter()
            frame(key)
            ms.setdefault(key, []).append((time.perf_counter() - t0) * 1e3)

    say("config 2, %dx%d, fuel %d, host pixels: ms per frame (wall clock), min / median / max over %d rounds; rays_shadow of one frame" % (W, H, FUEL, rounds))
    table = {}
    for (name, path), v in ms.items():
        table["%s | path %s" % (name, path)] = {"min": min(v), "median": statistics.median(v), "max": max(v), "rays_shadow": shadow[(name, path)]}
        say("  %-3s path %s  %9.3f / %9.3f / %9.3f   rays_shadow %12d" % (name, path, min(v), statistics.median(v), max(v), shadow[(name, path)]))
    checks = {}
    for path in ("1", "4"):
        same = bool(np.array_equal(pixels[("a", path)].view(np.uint64), pixels[("b", path)].view(np.uint64))) and shadow[("a", path)] == shadow[("b", path)]
        checks["b == a | path %s" % path] = same
        say("  path %s: frame b has frame a's bits and rays_shadow: %s" % (path, same))
    for name in frames:
        same = bool(np.array_equal(pixels[(name, "1")].view(np.uint64), pixels[(name, "4")].view(np.uint64)))
        checks["%s: path 1 == path 4" % name] = same
        say("  frame %-3s: both paths give the same bits: %s" % (name, same))

    bar = {}
    for path in ("1", "4"):
        a, b = table["a | path %s" % path], table["b | path %s" % path]
        allowed = a["median"] + (a["max"] - a["min"])
        bar["b | path %s" % path] = {"ms": b["median"], "allowed_ms": allowed, "a_median_ms": a["median"], "a_spread_ms": a["max"] - a["min"], "within": b["median"] <= allowed}
        say("bar, b path %s: %.3f ms; allowed %.3f ms = a's median %.3f + a's spread %.3f: %s" % (path, b["median"], allowed, a["median"], a["max"] - a["min"],
                                                                                                   "within" if b["median"] <= allowed else "OVER"))
        for name, ref in (("c", "a"), ("d", "d0")):
            x, r = table["%s | path %s" % (name, path)], table["%s | path %s" % (ref, path)]
            say("cone, %s path %s: %.3f ms against %s's %.3f ms (%.2f x); rays_shadow %d against %d (%.1f %%)" % (
                name, path, x["median"], ref, r["median"], x["median"] / r["median"], x["rays_shadow"], r["rays_shadow"], 100.0 * x["rays_shadow"] / max(1, r["rays_shadow"])))
    say(json.dumps({"rounds": rounds, "ms": table, "checks": checks, "bar": bar}))
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    args = sys.argv[1:]
    out = os.path.join(ROOT, "profiles", "spot_probe.txt")
    if "--out" in args:
        i = args.index("--out")
        out = args[i + 1]
        del args[i:i + 2]
    main(int(args[0]) if args else 7, out)
