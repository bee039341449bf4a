"""Test-only access to the CPU oracle (oracle/_build/liboracle.so).  Never imported by the product package."""
import ctypes as C
import os
import subprocess

import numpy as np

from raytracer_challenge_amd.backend import Backend, HIT_DTYPE

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ORACLE_DIR = os.path.join(ROOT, "oracle")
LIB = os.path.join(ORACLE_DIR, "_build", "liboracle.so")
KNOWN = os.path.join(ORACLE_DIR, "_build", "known_answers")


class OrcStats(C.Structure):
    _fields_ = [("seconds", C.c_double), ("threads", C.c_uint64), ("unique_rays", C.c_double), ("traced_rays", C.c_double), ("nan_seen", C.c_uint64)]


COUNT_ROWS = ("primary", "reflect", "refract", "shadow", "container", "calls_color_at", "calls_shadow")


class RayCounts(dict):
    """The oracle's ray counts by depth (oracle_capi.cpp orc_ray_counts): "primary", "reflect", "refract", "shadow", "container" count the
    de-duplicated tree, each ray (each hit, for container) once; "calls_color_at" and "calls_shadow" are the literal call counts, with
    the reference's per-light re-tracing.  Every value is a uint64 array indexed by depth."""

    def totals(self):
        """What include/rtc.h's rtc_stats reports: rays_primary, rays_shadow, rays_reflect, rays_refract, rays_container."""
        return {"rays_" + k: int(self[k].sum()) for k in ("primary", "shadow", "reflect", "refract", "container")}


def bind_ray_counts(lib):
    vp = C.c_void_p
    lib.orc_ray_count_depths.restype, lib.orc_ray_count_depths.argtypes = C.c_uint32, []
    lib.orc_ray_counts.restype, lib.orc_ray_counts.argtypes = C.c_int, [vp, vp, C.c_int, vp, C.c_uint64, C.c_uint32, vp]
    lib.orc_ray_counts_rays.restype, lib.orc_ray_counts_rays.argtypes = C.c_int, [vp, vp, C.c_uint64, C.c_int, vp]


def build_oracle():
    subprocess.run(["make", "-s", "-C", ORACLE_DIR], check=True)


class OracleBackend(Backend):
    def __init__(self):
        if not (os.path.exists(LIB) and os.path.exists(KNOWN)):
            build_oracle()
        super().__init__(LIB)
        assert self.name == "oracle-cpu"
        vp = C.c_void_p
        self.lib.orc_render.restype = C.c_int
        self.lib.orc_render.argtypes = [vp, vp, C.c_int, vp, C.c_uint64, vp, vp, C.c_uint32, C.POINTER(OrcStats)]
        self.lib.orc_render_ex.restype = C.c_int
        self.lib.orc_render_ex.argtypes = [vp, vp, C.c_int, vp, C.c_uint64, vp, vp, C.c_uint32, C.POINTER(OrcStats), vp]
        self.lib.orc_ppm.restype = C.c_uint64
        self.lib.orc_ppm.argtypes = [C.c_uint64, C.c_uint64, vp, C.c_char_p, C.c_uint64]
        self.lib.orc_quantize.restype = None
        self.lib.orc_quantize.argtypes = [vp, C.c_uint64, vp]
        self.lib.orc_simplex.restype = C.c_double
        self.lib.orc_simplex.argtypes = [C.c_double] * 3
        self.lib.orc_fractal.restype = C.c_double
        self.lib.orc_fractal.argtypes = [C.c_double] * 3 + [C.c_uint64]
        bind_ray_counts(self.lib)

    def render_timed(self, nw, camera, fuel, pixel_indices=None, threads=0):
        cam = self.camera_c(camera)
        if pixel_indices is None:
            n, idx_p = camera.hsize * camera.vsize, None
        else:
            pixel_indices = np.ascontiguousarray(pixel_indices, dtype=np.uint64)
            n, idx_p = pixel_indices.size, pixel_indices.ctypes.data
        rgb = np.empty((n, 3), dtype=np.float64)
        hits = np.empty(n, dtype=HIT_DTYPE)
        st = OrcStats()
        self._check(self.lib.orc_render(nw.handle, C.byref(cam), int(fuel), idx_p, n, rgb.ctypes.data, hits.ctypes.data, threads, C.byref(st)), "orc_render")
        return rgb, hits, st

    def render_with_digest(self, nw, camera, fuel, pixel_indices=None, threads=0):
        """One oracle pass: (rgb, primary hits, hit-tree digests) of the pixels."""
        cam = self.camera_c(camera)
        if pixel_indices is None:
            n, idx_p = camera.hsize * camera.vsize, None
        else:
            pixel_indices = np.ascontiguousarray(pixel_indices, dtype=np.uint64)
            n, idx_p = pixel_indices.size, pixel_indices.ctypes.data
        rgb = np.empty((n, 3), dtype=np.float64)
        hits = np.empty(n, dtype=HIT_DTYPE)
        dig = np.empty(n, dtype=np.uint64)
        self._check(self.lib.orc_render_ex(nw.handle, C.byref(cam), int(fuel), idx_p, n, rgb.ctypes.data, hits.ctypes.data, threads, None, dig.ctypes.data), "orc_render_ex")
        return rgb, hits, dig

    def _counts(self, out):
        return RayCounts(zip(COUNT_ROWS, out.copy()))

    def ray_counts(self, nw, camera, fuel, pixel_indices=None, threads=0):
        """RayCounts of the listed pixels (None: the whole frame; a pixel listed twice counts twice)."""
        cam = self.camera_c(camera)
        if pixel_indices is None:
            n, idx_p = camera.hsize * camera.vsize, None
        else:
            pixel_indices = np.ascontiguousarray(pixel_indices, dtype=np.uint64)
            n, idx_p = pixel_indices.size, pixel_indices.ctypes.data
        out = np.zeros((len(COUNT_ROWS), int(self.lib.orc_ray_count_depths())), dtype=np.uint64)
        self._check(self.lib.orc_ray_counts(nw.handle, C.byref(cam), int(fuel), idx_p, n, threads, out.ctypes.data), "orc_ray_counts")
        return self._counts(out)

    def ray_counts_rays(self, nw, rays, fuel):
        """RayCounts of explicit rays (what color_at takes)."""
        rays = np.ascontiguousarray(rays, dtype=np.float64).reshape(-1, 6)
        out = np.zeros((len(COUNT_ROWS), int(self.lib.orc_ray_count_depths())), dtype=np.uint64)
        self._check(self.lib.orc_ray_counts_rays(nw.handle, rays.ctypes.data, len(rays), int(fuel), out.ctypes.data), "orc_ray_counts_rays")
        return self._counts(out)

    def quantize(self, rgb):
        rgb = np.ascontiguousarray(rgb, dtype=np.float64)
        out = np.empty(rgb.shape, dtype=np.uint8)
        self.lib.orc_quantize(rgb.ctypes.data, rgb.size, out.ctypes.data)
        return out

    def ppm(self, hsize, vsize, rgb):
        rgb = np.ascontiguousarray(rgb, dtype=np.float64)
        need = self.lib.orc_ppm(hsize, vsize, rgb.ctypes.data, None, 0)
        buf = C.create_string_buffer(int(need) + 1)
        self.lib.orc_ppm(hsize, vsize, rgb.ctypes.data, buf, need + 1)
        return buf.value.decode()


_oracle = None


def oracle() -> OracleBackend:
    global _oracle
    if _oracle is None:
        _oracle = OracleBackend()
    return _oracle
