#!/usr/bin/env python3
"""Cost of normal perturbation (include/rtc.h rtc_bump) on config 2 and config 3 at 1920x1080, fuel 5, as HOST pixels (wall clock around
rtc_render), on each pinned device path.  ROUNDS rounds alternate over all frames in one process, so every figure has a run-to-run spread
(min / median / max over the rounds).  The frames, per config:
  smooth    the config as it is
  zero      every material with a fractal record (3 octaves) of amplitude 0: the NP builds run, the noise is evaluated, the pixels are the
            smooth frame's -- what leaving the scene's own builds costs, with the same rays
  bumped    every material with a fractal record (3 octaves) of amplitude 0.1, frequency 2: other reflections, so other rays too
The hit records of the three frames must be equal, zero's pixels and ray counters must be smooth's, and both paths must give the same
bits, which is checked here too.

    bump_probe.py [ROUNDS] [--out FILE]          (GPU; FILE defaults to profiles/bump_probe.txt)"""
import ctypes as C
import dataclasses
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
W, H, FUEL = 1920, 1080, 5


def with_bump(world, bump):
    from raytracer_challenge_amd.scene import World

    def mat(m):
        return None if m is None else dataclasses.replace(m, bump=bump)

    def el(e):
        if e.tag == "shape":
            return dataclasses.replace(e, args=dataclasses.replace(e.args, material=mat(e.args.material)))
        if e.tag == "composite":
            return dataclasses.replace(e, material=mat(e.material), children=tuple(el(c) for c in e.children))
        return dataclasses.replace(e, material=mat(e.material))
    return World(world.lights, [el(e) for e in world.elements], world.background)


def worlds():
    from raytracer_challenge_amd import scenes
    from raytracer_challenge_amd.scene import Bump
    out = {}
    for name, (cam, world) in (("config2", scenes.synthetic_analytic(n_primitives=512, seed=12345, cones=False, grouped=False, hsize=W, vsize=H)),
                               ("config3", scenes.chapter15_teapot("teapot_low.obj", W, H))):
        out[name] = (cam, {"smooth": world, "zero": with_bump(world, Bump.fractal(3, 0.0, 2.0)), "bumped": with_bump(world, Bump.fractal(3, 0.1, 2.0))})
    return out


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
    lib = be.lib
    vp = C.c_void_p
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
        pixels[key], records[key] = rgb.copy(), hits.copy()
    ms = {}
    for _ in range(rounds):
        for key in scene_of:
            t0 = time.perf_counter()
            frame(key)
            ms.setdefault(key, []).append((time.perf_counter() - t0) * 1e3)

    say("%dx%d, fuel %d, host pixels: ms per frame (wall clock), min / median / max over %d rounds; kernel_ms and rays of one counted frame" % (W, H, FUEL, rounds))
    table = {}
    for key, v in ms.items():
        c = counted[key]
        table[" | ".join(key)] = {"min": min(v), "median": statistics.median(v), "max": max(v), **c}
        say("  %-8s %-6s path %s  %9.3f / %9.3f / %9.3f   kernel_ms %8.3f   rays %d" % (
            key[0], key[1], key[2], min(v), statistics.median(v), max(v), c["kernel_ms"], c["rays_primary"] + c["rays_shadow"] + c["rays_reflect"] + c["rays_refract"]))
    checks = {}
    ray_keys = ("rays_primary", "rays_shadow", "rays_reflect", "rays_refract")
    for config in ("config2", "config3"):
        for path in ("1", "4"):
            s, z, b = (config, "smooth", path), (config, "zero", path), (config, "bumped", path)
            same = (records[s].tobytes() == records[z].tobytes() == records[b].tobytes() and np.array_equal(pixels[s].view(np.uint64), pixels[z].view(np.uint64)) and
                    all(counted[s][k] == counted[z][k] for k in ray_keys))
            checks["%s path %s: zero is smooth, bumped has its hits" % (config, path)] = bool(same)
            say("  %s path %s: zero has smooth's pixels, hit records and ray counters, bumped its hit records: %s" % (config, path, same))
            r = table[" | ".join(s)]
            for other in (z, b):
                x = table[" | ".join(other)]
                say("  %s path %s: %-6s %.3f ms against smooth %.3f ms (%.3f x; smooth's spread %.3f ms); kernel_ms %.3f against %.3f" % (
                    config, path, other[1], x["median"], r["median"], x["median"] / r["median"], r["max"] - r["min"], x["kernel_ms"], r["kernel_ms"]))
        for name in ("smooth", "zero", "bumped"):
            same = bool(np.array_equal(pixels[(config, name, "1")].view(np.uint64), pixels[(config, name, "4")].view(np.uint64)))
            checks["%s %s: path 1 == path 4" % (config, name)] = same
            say("  %s %-6s: both paths give the same bits: %s" % (config, name, same))
    say(json.dumps({"rounds": rounds, "ms": table, "checks": checks}))
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        f.write("\n".join(lines) + "\n")
    return 0 if all(checks.values()) else 1


if __name__ == "__main__":
    args = sys.argv[1:]
    out = os.path.join(ROOT, "profiles", "bump_probe.txt")
    if "--out" in args:
        k = args.index("--out")
        out = args[k + 1]
        del args[k:k + 2]
    sys.exit(main(int(args[0]) if args else 7, out))
