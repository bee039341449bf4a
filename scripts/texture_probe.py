#!/usr/bin/env python3
"""Cost of texture mapping (include/rtc.h RTC_PAT_UV) on config 2's scene, 1920x1080, fuel 5, on each device path, in four versions:
  plain     the scene as it is (Plain colours: the kernels without a pattern walk where the scene allows them);
  checkers  every surface's colour c as a 3D Checkers(c, c / 2) (the pattern-walking kernel instantiations);
  textured  planes planar-mapped UV checkers, spheres spherically mapped onto one 1024x512 image, cubes cube-mapped (align-check
            faces), cylinders cylindrically mapped UV checkers (the UV kernel instantiations).
  linear    textured with every image face looked up bilinearly (RTC_UV_IMAGE_LINEAR*, the wrap its map asks for).
textured - checkers is the cost of the UV lookups; checkers - plain that of the pattern-walking kernels every patterned scene runs;
linear - textured that of three more texel gathers per lookup.
ms per frame: device time between stream markers around K asynchronous whole-frame launches; with --repeats R that is measured R times
per row (after the warm-up) and the median, the least and the greatest are printed: max - min is the resolution of a comparison
between two builds of the library (RTC_AMD_LIB names another build; --rows leaves out rows an older build cannot create).

usage: texture_probe.py [K] [--repeats R] [--rows plain,checkers,textured,linear]      (GPU)
       texture_probe.py --resource-usage    (no GPU: `make resource-usage VARIANTS="8 9"`, the UV instantiations)"""
import ctypes as C
import json
import os
import re
import subprocess
import sys
from dataclasses import replace

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
CSRC = os.path.join(ROOT, "raytracer_challenge_amd", "csrc")


def resource_usage():
    out = subprocess.run(["make", "-s", "-C", CSRC, "resource-usage", "VARIANTS=8 9"], check=True, stdout=subprocess.PIPE, text=True).stdout
    # the UV builds: the instantiations of rtc_trace_kernel (variants 8 and 9) whose seventh template argument, UV, is true, and of
    # wf_shade whose third is (the other kernels of rtc_kernels.hip are not)
    uv = re.compile(r"_uv|rtc_trace_kernelI(L[bi]\d+E){6}Lb1E|wf_shadeI(Lb\dE){2}Lb1E")
    for line in out.splitlines():
        if uv.search(line):
            print("  " + "  ".join(f for f in line.split("\t") if "LDS" not in f))


def versions():
    import numpy as np
    from raytracer_challenge_amd import Texture, UvPattern, scenes
    from raytracer_challenge_amd.scene import Color, Matrix, Pattern, World
    cam, world = scenes.synthetic_analytic(n_primitives=512, seed=12345, cones=False, grouped=False, hsize=1920, vsize=1080)
    rng = np.random.RandomState(5)
    image = Texture(rng.uniform(0.0, 1.0, size=(512, 1024, 3)))

    def repattern(how):
        out = []
        for e in world.elements:
            c = e.args.material.pattern.color
            a, b = Pattern.plain(c), Pattern.plain(Color(c.r * 0.5, c.g * 0.5, c.b * 0.5))
            p = how(e.geometry, a, b)
            out.append(replace(e, args=replace(e.args, material=replace(e.args.material, pattern=p))))
        return World(world.lights, out)

    def checkers(geom, a, b):
        return Pattern.checkers(Matrix.scaling(0.5, 0.5, 0.5), a, b)

    def textured(geom, a, b, filter="nearest"):
        if geom == "plane":
            return Pattern.texture_map(Matrix.scaling(2.0, 2.0, 2.0), "planar", UvPattern.checkers(2.0, 2.0, a, b))
        if geom == "sphere":
            return Pattern.texture_map(Matrix.id(), "spherical", UvPattern.image(image, filter=filter))
        if geom == "cylinder":
            return Pattern.texture_map(Matrix.id(), "cylindrical", UvPattern.checkers(8.0, 2.0, a, b))
        return Pattern.cube_map(Matrix.id(), *[UvPattern.align_check(a, b, b, b, b)] * 6)
    return cam, [("plain", lambda: world), ("checkers", lambda: repattern(checkers)), ("textured", lambda: repattern(textured)),
                 ("linear", lambda: repattern(lambda g, a, b: textured(g, a, b, "linear")))]


def main(k, repeats=1, rows=("plain", "checkers", "textured", "linear")):
    import numpy as np
    import torch
    import raytracer_challenge_amd as rt
    from raytracer_challenge_amd.device import RtcStatsC

    cam, worlds = versions()
    be = rt.hip_backend()
    lib = be.lib
    vp = C.c_void_p
    n = cam.hsize * cam.vsize
    rc_cam = be._rtc_camera(cam)
    out = torch.empty(n * 3, dtype=torch.float64, device="cuda:0")
    rgb = np.empty((n, 3))
    results = {}
    for label, make_world in worlds:
        if label not in rows:
            continue
        w = make_world()
        for path in ("1", "4"):
            os.environ["RTC_KERNEL"] = path
            nw = be.build_world(w)
            scene = lib.rtw_world_scene(nw.handle, 0)
            assert scene, be._err()
            st = RtcStatsC()
            assert lib.rtc_render(scene, rc_cam, 5, None, 0, n, rgb.ctypes.data, None, C.byref(st)) == 0, lib.rtc_last_error()
            for _ in range(2):   # warm-up: code loading, queues
                assert lib.rtc_render_rows_device(scene, rc_cam, 5, 0, 1, cam.vsize, C.c_void_p(out.data_ptr()), None, 0, 1) == 0, lib.rtc_last_error()
            runs = []
            for _ in range(repeats):
                assert lib.rtc_scene_record(scene, 0) == 0
                for _ in range(k):
                    assert lib.rtc_render_rows_device(scene, rc_cam, 5, 0, 1, cam.vsize, C.c_void_p(out.data_ptr()), None, 0, 0) == 0, lib.rtc_last_error()
                assert lib.rtc_scene_record(scene, 1) == 0 and lib.rtc_scene_wait(scene, 1) == 0
                ms = C.c_double()
                assert lib.rtc_scene_elapsed_ms(scene, 0, 1, C.byref(ms)) == 0
                runs.append(ms.value / k)
            per = sorted(runs)[len(runs) // 2]
            rays = st.rays_primary + st.rays_reflect + st.rays_refract
            results["%s_path%s" % (label, path)] = {"ms_per_frame": per, "runs": runs, "shaded_rays": rays, "device_bytes": lib.rtc_scene_device_bytes(scene)}
            spread = "  (min %.2f max %.2f over %d)" % (min(runs), max(runs), repeats) if repeats > 1 else ""
            print("%-9s path %s: %8.2f ms/frame%s  %6.1f M camera + secondary rays  %8.1f MB on the device" % (
                label, path, per, spread, rays / 1e6, lib.rtc_scene_device_bytes(scene) / 1e6), flush=True)
            nw.close()
    for path in ("1", "4"):
        ms = {v: results["%s_path%s" % (v, path)]["ms_per_frame"] for v in rows}
        parts = ["%s - %s %+.2f ms (%+.1f %%)" % (a, b, ms[a] - ms[b], 100 * (ms[a] - ms[b]) / ms[b])
                 for a, b in (("checkers", "plain"), ("textured", "checkers"), ("linear", "textured")) if a in ms and b in ms]
        if parts:
            print("path %s: %s" % (path, ", ".join(parts)))
    print(json.dumps({"k": k, "repeats": repeats, "results": results}))


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "--resource-usage":
        resource_usage()
    else:
        import argparse
        ap = argparse.ArgumentParser()
        ap.add_argument("k", nargs="?", type=int, default=10)
        ap.add_argument("--repeats", type=int, default=1)
        ap.add_argument("--rows", default="plain,checkers,textured,linear")
        a = ap.parse_args()
        main(a.k, a.repeats, tuple(a.rows.split(",")))
