#!/usr/bin/env python3
"""Cost of area lights (include/rtc.h rtc_light_ex) on config 2's scene: every point light replaced by a 4x4 jittered area light
(2 x 2 units, centred on the light), 1920x1080, fuel 5, on each device path, beside the point-light frame.  Reports ms per frame
(device time between stream markers around K asynchronous whole-frame launches), shadow rays per frame (one counting launch), Grays/s
of shadow rays, ns per shadow ray, and the path the library picks on its own (RTC_KERNEL unset).

The cost of one more shadow ray of each kind is measured the same way for both, as extra frame time over extra shadow rays (each
extra ray brings its Phong terms along): point-light rays between config 2 and config 2 with every light doubled (two lights of half
the intensity at the same place: grid-served rays on the point-light kernels); area-light sample rays between 2x2 and 4x4 lights
(the same area kernels, 12 more samples per light).

usage: area_light_probe.py [K]                 (GPU)
       area_light_probe.py --resource-usage    (no GPU: `make resource-usage VARIANTS="6 7"`, the area-light instantiations)"""
import ctypes as C
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
CSRC = os.path.join(ROOT, "raytracer_challenge_amd", "csrc")


def resource_usage():
    out = subprocess.run(["make", "-s", "-C", CSRC, "resource-usage", "VARIANTS=6 7"], check=True, stdout=subprocess.PIPE, text=True).stdout
    for line in out.splitlines():   # (the variant-independent kernels of rtc_kernels.hip follow; they are not area-light builds)
        if "rtc_trace_kernel" in line or "wf_ts" in line:
            print("  " + "  ".join(f for f in line.split("\t") if "LDS" not in f))


def main(k):
    import numpy as np
    import torch
    import raytracer_challenge_amd as rt
    from raytracer_challenge_amd import scenes
    from raytracer_challenge_amd.device import RtcStatsC
    from raytracer_challenge_amd.scene import AreaLight, Color, PointLight, Vector, World

    cam, world = scenes.synthetic_analytic(n_primitives=512, seed=12345, cones=False, grouped=False, hsize=1920, vsize=1080)

    def area(n):
        return World([AreaLight(l.intensity, Vector.point(l.origin[0] - 1.0, l.origin[1], l.origin[2] - 1.0), Vector.vector(2.0, 0.0, 0.0), n,
                                Vector.vector(0.0, 0.0, 2.0), n, True) for l in world.lights], world.elements)
    half = [PointLight(Color(l.intensity.r * 0.5, l.intensity.g * 0.5, l.intensity.b * 0.5), l.origin) for l in world.lights]
    doubled = World([h for h in half for _ in range(2)], world.elements)
    be = rt.hip_backend()
    lib = be.lib
    vp = C.c_void_p
    n = cam.hsize * cam.vsize
    rc_cam = be._rtc_camera(cam)
    out = torch.empty(n * 3, dtype=torch.float64, device="cuda:0")
    rgb = np.empty((n, 3))
    results = {}
    for label, w in (("point", world), ("point_doubled", doubled), ("area2x2", area(2)), ("area4x4", area(4))):
        for path in ("1", "4", "auto") if label in ("point", "area4x4") else ("1", "4"):
            if path == "auto":
                os.environ.pop("RTC_KERNEL", None)
            else:
                os.environ["RTC_KERNEL"] = path
            nw = be.build_world(w)
            scene = lib.rtw_world_scene(nw.handle, 0)
            assert scene, be._err()
            st = RtcStatsC()
            assert lib.rtc_render(scene, rc_cam, 5, None, 0, n, rgb.ctypes.data, None, C.byref(st)) == 0, lib.rtc_last_error()
            if path == "auto":   # the measured choice: two synchronous launches per path, then the faster
                for _ in range(4):
                    assert lib.rtc_render(scene, rc_cam, 5, None, 0, n, rgb.ctypes.data, None, None) == 0, lib.rtc_last_error()
                ch, m1, m4 = C.c_int32(), C.c_double(), C.c_double()
                lib.rtc_scene_path_info(scene, C.byref(ch), C.byref(m1), C.byref(m4))
                results["%s_choice" % label] = {"path": ch.value, "one_kernel_ms": m1.value, "wavefront_ms": m4.value}
                print("%-13s library's choice: path %d (one kernel %.2f ms, wavefront %.2f ms)" % (label, ch.value, m1.value, m4.value), flush=True)
                nw.close()
                continue
            for _ in range(2):   # warm-up: code loading, queues
                assert lib.rtc_render_rows_device(scene, rc_cam, 5, 0, 1, cam.vsize, C.c_void_p(out.data_ptr()), None, 0, 1) == 0, lib.rtc_last_error()
            assert lib.rtc_scene_record(scene, 0) == 0
            for _ in range(k):
                assert lib.rtc_render_rows_device(scene, rc_cam, 5, 0, 1, cam.vsize, C.c_void_p(out.data_ptr()), None, 0, 0) == 0, lib.rtc_last_error()
            assert lib.rtc_scene_record(scene, 1) == 0 and lib.rtc_scene_wait(scene, 1) == 0
            ms = C.c_double()
            assert lib.rtc_scene_elapsed_ms(scene, 0, 1, C.byref(ms)) == 0
            per = ms.value / k
            r = {"ms_per_frame": per, "rays_shadow": st.rays_shadow, "rays_primary": st.rays_primary, "rays_reflect": st.rays_reflect,
                 "rays_refract": st.rays_refract, "light_grid_cells": st.light_grid_cells, "shadow_grays_s": st.rays_shadow / (per * 1e-3) / 1e9,
                 "ns_per_shadow_ray_upper_bound": per * 1e6 / st.rays_shadow}
            results["%s_path%s" % (label, path)] = r
            print("%-13s path %s: %8.2f ms/frame  %6.1f M shadow rays  %6.2f Grays/s (shadow rays / frame time)  %.3f ns/shadow ray (whole frame)  grid cells %d"
                  % (label, path, per, st.rays_shadow / 1e6, r["shadow_grays_s"], r["ns_per_shadow_ray_upper_bound"], st.light_grid_cells), flush=True)
            nw.close()

    def marginal(hi, lo):
        a, b = results[hi], results[lo]
        return (a["ms_per_frame"] - b["ms_per_frame"]) * 1e6 / max(1, a["rays_shadow"] - b["rays_shadow"]), (a["rays_shadow"] - b["rays_shadow"]) / 1e6
    for path in ("1", "4"):
        pt, npt = marginal("point_doubled_path%s" % path, "point_path%s" % path)
        ar, nar = marginal("area4x4_path%s" % path, "area2x2_path%s" % path)
        results["path%s_ns_per_extra_point_shadow_ray" % path], results["path%s_ns_per_extra_area_shadow_ray" % path] = pt, ar
        print("path %s: one more shadow ray (extra frame time / extra rays, Phong terms included): point light %.4f ns (%.1f M more), area-light "
              "sample %.4f ns (%.1f M more): ratio %.2f" % (path, pt, npt, ar, nar, ar / pt))
    print(json.dumps({"k": k, "results": results}))


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "--resource-usage":
        resource_usage()
    else:
        main(int(sys.argv[1]) if len(sys.argv) > 1 else 10)
