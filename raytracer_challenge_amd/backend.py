"""ctypes binding of include/rtw.h — generic over the library that implements it.

``Backend(path)`` loads one shared library exporting the ``rtw_*`` symbols and turns the pure-Python
scene description (:mod:`raytracer_challenge_amd.scene`) into native handles.  The package itself only
ever loads its own HIP library (:func:`raytracer_challenge_amd.hip_backend`); tests load the CPU oracle
through this same class from ``tests/`` — the product never does.
"""
from __future__ import annotations

import ctypes as C
import os
from typing import Dict, Optional, Sequence

import numpy as np

from .scene import (BACKGROUND_PROJECTIONS, BUMP_KINDS, FUEL, GEOMETRY, GROUP_KINDS, JITTER_KINDS, MIXTURE_KINDS, Adaptive, AreaLight, Camera, Cone, Element, FILTER_KINDS, Filter, Material, Pattern, SHUTTER_MAX_POSES, Sampling, Shutter, World)
from .cabi import HIT_DTYPE, AdaptiveC, CameraC, FilterC, MaterialC as _MaterialC, SamplingC, ShutterC, UvFaceC as _UvFaceC, RtcCameraC, bind  # noqa: F401
from .texture import UV_MAPS, Texture


class RtwError(RuntimeError):
    pass


RTW_SYMBOLS = [
    "rtw_last_error", "rtw_backend", "rtw_pattern_debug", "rtw_pattern_plain", "rtw_pattern_jitter", "rtw_pattern_mixture",
    "rtw_pattern_release", "rtw_shape", "rtw_composite", "rtw_parse_obj", "rtw_element_release", "rtw_world_create",
    "rtw_world_add_light", "rtw_world_add_element", "rtw_world_primitive_count", "rtw_world_release", "rtw_render", "rtw_color_at",
]


def _d16(m) -> C.Array:
    return (C.c_double * 16)(*m.flat())


class NativeWorld:
    """Owns one ``rtw_world*``."""

    def __init__(self, backend: "Backend", handle: int, n_lights: int):
        self.backend, self.handle, self.n_lights = backend, handle, n_lights

    @property
    def primitive_count(self) -> int:
        return int(self.backend._lib.rtw_world_primitive_count(self.handle))

    def close(self):
        if self.handle:
            self.backend._lib.rtw_world_release(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Backend:
    def __init__(self, lib_path: str):
        if not os.path.exists(lib_path):
            raise RtwError("native library not found: %s (run `python -c 'import __graft_entry__ as g; g.build()'`)" % lib_path)
        self.path = lib_path
        # two handles on the one loaded library, each with its own function objects.  `lib` is for callers of the raw entry points
        # (tests, probes, bench.py): whatever they assign to its argtypes afterwards cannot reach the package's own calls, which
        # go through `_lib` and rely on the table's types.
        self.lib = bind(C.CDLL(lib_path))
        self._lib = lib = bind(C.CDLL(lib_path))
        for name in RTW_SYMBOLS:
            getattr(lib, name)  # AttributeError = missing export: fail loudly
        self.name = lib.rtw_backend().decode()
        # the product library's extensions of rtw.h (the oracle restates the reference, which has none)
        self.has_area_lights = hasattr(lib, "rtw_world_add_area_light")
        self.has_light_cones = hasattr(lib, "rtw_world_set_light_cone")
        self.has_background = hasattr(lib, "rtw_world_set_background")
        self.has_bump = hasattr(lib, "rtw_element_set_bump")
        self.has_texture_map = hasattr(lib, "rtw_pattern_uv")

    # ---- errors
    def _err(self) -> str:
        return (self._lib.rtw_last_error() or b"").decode()

    def _check_ptr(self, p, what):
        if not p:
            raise RtwError("%s failed: %s" % (what, self._err()))
        return p

    def _check(self, rc, what):
        if rc != 0:
            raise RtwError("%s failed: %s" % (what, self._err()))

    # ---- scene -> handles
    def _pattern(self, p: Pattern, cache: Dict[int, int], owned: list) -> int:
        key = id(p)
        if key in cache:
            return cache[key]
        lib = self._lib
        if p.tag == "debug":
            h = lib.rtw_pattern_debug()
        elif p.tag == "plain":
            h = lib.rtw_pattern_plain(p.color.r, p.color.g, p.color.b)
        elif p.tag == "jitter":
            child = self._pattern(p.left, cache, owned)
            h = lib.rtw_pattern_jitter(JITTER_KINDS[p.kind], 1 if p.noise.kind == "fractal" else 0, p.noise.scale, p.noise.octaves, child)
        elif p.tag == "mixture":
            l, r = self._pattern(p.left, cache, owned), self._pattern(p.right, cache, owned)
            h = lib.rtw_pattern_mixture(MIXTURE_KINDS[p.kind], _d16(p.transform), l, r)
        elif p.tag == "uv":
            if not self.has_texture_map:
                raise RtwError("texture-mapped patterns need librtc_amd.so (backend %r has no rtw_pattern_uv)" % self.name)
            faces = (_UvFaceC * len(p.faces))()
            for k, f in enumerate(p.faces):
                faces[k].kind, faces[k].width, faces[k].height = f.kind_code(p.kind), f.width, f.height
                faces[k].texture = self._texture(f.texture, cache, owned) if f.texture is not None else None
                for c, child in enumerate(f.children):
                    faces[k].child[c] = self._pattern(child, cache, owned)
            h = lib.rtw_pattern_uv(UV_MAPS[p.kind], _d16(p.transform), faces, len(p.faces))
        else:
            raise RtwError("unknown pattern tag %r" % (p.tag,))
        self._check_ptr(h, "pattern")
        cache[key] = h
        owned.append(h)
        return h

    def _texture(self, t: Texture, cache, owned) -> int:
        key = ("texture", id(t))
        if key not in cache:
            rgb = np.ascontiguousarray(t.rgb, dtype=np.float64)
            h = self._check_ptr(self._lib.rtw_texture_create(t.width, t.height, rgb.ctypes.data), "texture")
            cache[key] = h
            owned.append(("texture", h))
        return cache[key]

    def _material(self, m: Material, cache, owned) -> _MaterialC:
        return _MaterialC(m.ambient, m.diffuse, m.specular, m.shininess, m.reflective, m.transparency, m.refractive_index,
                          self._pattern(m.pattern, cache, owned))

    def _bump(self, h: int, m: Optional[Material]) -> int:
        """The material's bump, if it has one, on every primitive of element `h` (include/rtw.h rtw_element_set_bump)."""
        b = getattr(m, "bump", None)
        if b is None:
            return h
        if not self.has_bump:
            self._lib.rtw_element_release(h)
            raise RtwError("a bump needs librtc_amd.so (backend %r has no rtw_element_set_bump)" % self.name)
        if self._lib.rtw_element_set_bump(h, BUMP_KINDS.index(b.kind), int(b.octaves), float(b.amplitude), float(b.frequency)) != 0:
            msg = self._err()
            self._lib.rtw_element_release(h)
            raise RtwError("set_bump failed: %s" % msg)
        return h

    def _element(self, e: Element, cache, owned) -> int:
        lib = self._lib
        if e.tag == "shape":
            mat = self._material(e.args.material, cache, owned)
            params = (C.c_double * max(1, len(e.params)))(*e.params)
            h = lib.rtw_shape(GEOMETRY[e.geometry], _d16(e.args.transform), C.byref(mat), 1 if e.args.casts_shadow else 0, params, len(e.params))
            return self._bump(self._check_ptr(h, "shape"), e.args.material)
        if e.tag == "composite":
            kids = [self._element(c, cache, owned) for c in e.children]
            arr = (C.c_void_p * max(1, len(kids)))(*kids)
            mat = self._material(e.material, cache, owned) if e.material is not None else None
            h = lib.rtw_composite(_d16(e.transform), C.byref(mat) if mat is not None else None, GROUP_KINDS[e.kind], arr, len(kids))
            return self._bump(self._check_ptr(h, "composite"), e.material)
        if e.tag == "obj":
            mat = self._material(e.material, cache, owned)
            ign, tris = C.c_uint64(0), C.c_uint64(0)
            h = lib.rtw_parse_obj(e.path.encode(), _d16(e.transform), C.byref(mat), C.byref(ign), C.byref(tris))
            return self._bump(self._check_ptr(h, "parse_obj(%s)" % e.path), e.material)
        raise RtwError("unknown element tag %r" % (e.tag,))

    def build_world(self, world: World) -> NativeWorld:
        lib = self._lib
        w = self._check_ptr(lib.rtw_world_create(), "world_create")
        cache: Dict[int, int] = {}
        owned: list = []
        try:
            for k, l in enumerate(world.lights):
                inten = (C.c_double * 3)(l.intensity.r, l.intensity.g, l.intensity.b)
                cone: Optional[Cone] = getattr(l, "cone", None)
                if cone is not None and not self.has_light_cones:
                    raise RtwError("light cones need librtc_amd.so (backend %r has no rtw_world_set_light_cone)" % self.name)
                if isinstance(l, AreaLight):
                    if not self.has_area_lights:
                        raise RtwError("area lights need librtc_amd.so (backend %r has no rtw_world_add_area_light)" % self.name)
                    v3 = lambda v: (C.c_double * 3)(*v[:3])  # noqa: E731
                    self._check(lib.rtw_world_add_area_light(w, inten, v3(l.corner), v3(l.uvec), int(l.usteps), v3(l.vvec), int(l.vsteps),
                                                             1 if l.jitter else 0), "add_area_light")
                else:
                    org = (C.c_double * 3)(*l.origin[:3])
                    self._check(lib.rtw_world_add_light(w, inten, org), "add_light")
                if cone is not None:
                    axis = (C.c_double * 3)(*cone.direction[:3])
                    self._check(lib.rtw_world_set_light_cone(w, k, axis, cone.cos_inner, cone.cos_outer), "set_light_cone")
            for e in world.elements:
                self._check(lib.rtw_world_add_element(w, self._element(e, cache, owned)), "add_element")
            bg = getattr(world, "background", None)
            if bg is not None:
                if not self.has_background:
                    raise RtwError("a background needs librtc_amd.so (backend %r has no rtw_world_set_background)" % self.name)
                self._check(lib.rtw_world_set_background(w, self._pattern(bg.pattern, cache, owned), BACKGROUND_PROJECTIONS.index(bg.projection)), "set_background")
        except Exception:
            lib.rtw_world_release(w)
            raise
        finally:
            for h in owned:
                if isinstance(h, tuple):
                    lib.rtw_texture_release(h[1])
                else:
                    lib.rtw_pattern_release(h)
        return NativeWorld(self, w, len(world.lights))

    # ---- the path
    @staticmethod
    def camera_c(camera: Camera) -> CameraC:
        c = CameraC()
        c.hsize, c.vsize, c.field_of_view = camera.hsize, camera.vsize, camera.field_of_view
        c.transform = _d16(camera.transform_matrix)
        return c

    def render(self, nw: NativeWorld, camera: Camera, fuel: int = FUEL, pixel_indices: Optional[np.ndarray] = None, want_hits: bool = True):
        """Image::par_render over all pixels (row-major) or the listed pixel indices.  Returns (rgb[n,3], hits[n])."""
        cam = self.camera_c(camera)
        n, idx_p, _keep = self._pixels(pixel_indices, camera.hsize * camera.vsize)
        rgb = np.empty((n, 3), dtype=np.float64)
        hits = np.empty(n, dtype=HIT_DTYPE) if want_hits else None
        self._check(self._lib.rtw_render(nw.handle, cam, int(fuel), idx_p, n, rgb.ctypes.data, hits.ctypes.data if want_hits else None), "render")
        return rgb, hits

    @staticmethod
    def _pixels(pixel_indices: Optional[np.ndarray], n_all):
        """(n, address or None, the array that owns the address) of a pixel list; None lists every pixel."""
        if pixel_indices is None:
            return n_all, None, None
        pixel_indices = np.ascontiguousarray(pixel_indices, dtype=np.uint64)
        return pixel_indices.size, pixel_indices.ctypes.data, pixel_indices

    def _scene(self, nw: Optional[NativeWorld], device: int):
        """The world's rtc_scene* on `device` (flattened and uploaded at the first request); None for no world."""
        if nw is None:
            return None
        scene = self._lib.rtw_world_scene(nw.handle, int(device))
        if not scene:
            raise RtwError("scene upload failed: %s" % self._err())
        return scene

    def _need(self, what: str, *symbols: str):
        """RtwError for a library without `symbols` (the CPU emulator, the oracle); the message names the first."""
        if not all(hasattr(self._lib, s) for s in symbols):
            raise RtwError("%s librtc_amd.so (backend %r has no %s)" % (what, self.name, symbols[0]))
        return self._lib

    def _rtc(self, rc, what):
        if rc != 0:
            raise RtwError("%s: %s" % (what, (self._lib.rtc_last_error() or b"").decode()))

    def _rtc_camera(self, camera: Camera, out: Optional[RtcCameraC] = None) -> RtcCameraC:
        out = RtcCameraC() if out is None else out
        if self._lib.rtw_make_camera(self.camera_c(camera), out) != 0:
            raise RtwError("camera: %s" % self._err())
        return out

    def render_digest(self, nw: NativeWorld, camera: Camera, fuel: int = FUEL, pixel_indices: Optional[np.ndarray] = None, device: int = 0) -> np.ndarray:
        """include/rtc.h rtc_render_hit_digest: per pixel, the digest of every closest hit of its ray tree (parity channel)."""
        scene = self._scene(nw, device)
        n, idx_p, _keep = self._pixels(pixel_indices, camera.hsize * camera.vsize)
        out = np.empty(n, dtype=np.uint64)
        self._rtc(self._lib.rtc_render_hit_digest(scene, self._rtc_camera(camera), int(fuel), idx_p, 0, n, out.ctypes.data), "rtc_render_hit_digest")
        return out

    def render_sampled(self, nw: NativeWorld, camera: Camera, sampling: Sampling, fuel: int = FUEL, pixel_indices: Optional[np.ndarray] = None,
                       device: int = 0) -> np.ndarray:
        """include/rtc.h rtc_render_sampled: every pixel (row-major) or the listed pixel indices as the mean of `sampling`'s rays.
        Returns rgb[n,3]."""
        lib = self._need("sampled cameras need", "rtc_render_sampled", "rtc_camera_rays")
        scene = self._scene(nw, device)
        rc_cam, sp = self._rtc_camera(camera), SamplingC.of(sampling)
        n, idx_p, _keep = self._pixels(pixel_indices, camera.hsize * camera.vsize)
        rgb = np.empty((n, 3), dtype=np.float64)
        self._rtc(lib.rtc_render_sampled(scene, rc_cam, sp, int(fuel), idx_p, 0, n, rgb.ctypes.data, None), "rtc_render_sampled")
        return rgb

    def camera_rays(self, camera: Camera, sampling: Sampling, pixel_indices: Optional[np.ndarray] = None, nw: Optional[NativeWorld] = None,
                    device: int = 0) -> np.ndarray:
        """include/rtc.h rtc_camera_rays: the sample rays {o, d} of every pixel or of the listed ones, [n, side*side, 6].  With a world
        they come from the device's generator kernel, without one from the same function evaluated on the host (no GPU needed)."""
        lib = self._need("sampled cameras need", "rtc_render_sampled", "rtc_camera_rays")
        scene = self._scene(nw, device)
        rc_cam, sp = self._rtc_camera(camera), SamplingC.of(sampling)
        n, idx_p, _keep = self._pixels(pixel_indices, camera.hsize * camera.vsize)
        rays = np.empty((n, sampling.samples, 6), dtype=np.float64)
        self._rtc(lib.rtc_camera_rays(scene, rc_cam, sp, idx_p, 0, n, rays.ctypes.data), "rtc_camera_rays")
        return rays

    def render_adaptive(self, nw: NativeWorld, camera: Camera, adaptive: Adaptive, fuel: int = FUEL, want_mask: bool = False, device: int = 0):
        """include/rtc.h rtc_render_adaptive: the whole frame, base pass plus the refined pixels' fine pass.  Returns rgb[n,3] or, with
        want_mask, (rgb[n,3], mask[n] of bool: the refined pixels)."""
        lib = self._need("adaptive sampling needs", "rtc_render_adaptive", "rtc_contrast_pixels")
        scene = self._scene(nw, device)
        rc_cam, ad = self._rtc_camera(camera), AdaptiveC.of(adaptive)
        n = camera.hsize * camera.vsize
        rgb = np.empty((n, 3), dtype=np.float64)
        mask = np.zeros(n, dtype=np.uint8) if want_mask else None
        self._rtc(lib.rtc_render_adaptive(scene, rc_cam, ad, int(fuel), rgb.ctypes.data, mask.ctypes.data if want_mask else None, None, None), "rtc_render_adaptive")
        return (rgb, mask.astype(bool)) if want_mask else rgb

    def contrast_pixels(self, frame: np.ndarray, hsize: int, vsize: int, threshold: float, neighbours: int = 4, nw: Optional[NativeWorld] = None,
                        device: int = 0) -> np.ndarray:
        """include/rtc.h rtc_contrast_pixels: the image indices (ascending, uint64) of the pixels of `frame` (hsize*vsize rows of r, g, b)
        that adaptive sampling would refine.  With a world the device kernels flag and compact them, without one the same function
        is evaluated on the host (no GPU needed)."""
        lib = self._need("adaptive sampling needs", "rtc_render_adaptive", "rtc_contrast_pixels")
        scene = self._scene(nw, device)
        frame = np.ascontiguousarray(frame, dtype=np.float64)
        if frame.size != int(hsize) * int(vsize) * 3:
            raise ValueError("frame must hold hsize * vsize * 3 values")
        out = np.empty(max(1, int(hsize) * int(vsize)), dtype=np.uint64)
        n = C.c_uint64(0)
        self._rtc(lib.rtc_contrast_pixels(scene, int(hsize), int(vsize), frame.ctypes.data, float(threshold), int(neighbours), out.ctypes.data, C.byref(n)),
                  "rtc_contrast_pixels")
        return out[:n.value].copy()

    def render_filtered(self, nw: NativeWorld, camera: Camera, sampling: Sampling, filter: Filter, fuel: int = FUEL, row_first: int = 0,
                        n_rows: Optional[int] = None, device: int = 0) -> np.ndarray:
        """include/rtc.h rtc_render_filtered: the rows row_first .. row_first + n_rows - 1 (default: to the last row) of the frame, every
        pixel the `filter`-weighted mean of `sampling`'s samples around it -- neighbours outside the row range included.  Returns rgb[n,3]."""
        lib = self._need("reconstruction filters need", "rtc_render_filtered", "rtc_filter_frame")
        scene = self._scene(nw, device)
        rc_cam, sp, fl = self._rtc_camera(camera), SamplingC.of(sampling), FilterC.of(filter)
        if n_rows is None:
            n_rows = camera.vsize - int(row_first)
        rgb = np.empty((max(0, int(n_rows)) * camera.hsize, 3), dtype=np.float64)
        self._rtc(lib.rtc_render_filtered(scene, rc_cam, sp, fl, int(fuel), int(row_first), int(n_rows), rgb.ctypes.data, None), "rtc_render_filtered")
        return rgb

    def filter_frame(self, samples: np.ndarray, hsize: int, vsize: int, sampling: Sampling, filter: Filter, nw: Optional[NativeWorld] = None,
                     device: int = 0) -> np.ndarray:
        """include/rtc.h rtc_filter_frame: the filter step alone over `samples` (hsize*vsize*side*side rows of r, g, b: pixel-major, k
        inner).  With a world the device kernel filters them, without one the same function is evaluated on the host (no GPU needed).
        Returns rgb[hsize*vsize,3]."""
        lib = self._need("reconstruction filters need", "rtc_render_filtered", "rtc_filter_frame")
        scene = self._scene(nw, device)
        samples = np.ascontiguousarray(samples, dtype=np.float64)
        if samples.size != int(hsize) * int(vsize) * sampling.samples * 3:
            raise ValueError("samples must hold hsize * vsize * side * side * 3 values")
        sp, fl = SamplingC.of(sampling), FilterC.of(filter)
        rgb = np.empty((int(hsize) * int(vsize), 3), dtype=np.float64)
        self._rtc(lib.rtc_filter_frame(scene, int(hsize), int(vsize), sp, fl, samples.ctypes.data, rgb.ctypes.data), "rtc_filter_frame")
        return rgb

    def render_shutter(self, nws: Sequence[NativeWorld], cameras: Sequence[Camera], sampling: Sampling, shutter: Shutter, fuel: int = FUEL,
                       pixel_indices: Optional[np.ndarray] = None, stats=None, device: int = 0) -> np.ndarray:
        """include/rtc.h rtc_render_shutter: pose p is (nws[p], cameras[p]); every pixel (row-major) or the listed pixel indices as the
        mean of `sampling`'s rays, each traced in the pose `shutter` deals it to.  A world given several times is one scene.  stats: an
        rtc_stats structure (ctypes) to fill.  Returns rgb[n,3]."""
        if len(nws) != len(cameras):
            raise ValueError("render_shutter: as many worlds as cameras")
        if not 1 <= len(nws) <= SHUTTER_MAX_POSES:
            raise ValueError("render_shutter: 1 to %d poses" % SHUTTER_MAX_POSES)
        if any((c.hsize, c.vsize) != (cameras[0].hsize, cameras[0].vsize) for c in cameras):
            raise ValueError("render_shutter: the cameras' hsize or vsize differ")
        lib = self._need("a shutter needs", "rtc_render_shutter", "rtc_shutter_deal")
        K = len(nws)
        scenes = (C.c_void_p * K)(*[self._scene(nw, device) for nw in nws])
        cams = (RtcCameraC * K)()
        for p, cam in enumerate(cameras):
            self._rtc_camera(cam, cams[p])
        sp, sh = SamplingC.of(sampling), ShutterC.of(shutter)
        n, idx_p, _keep = self._pixels(pixel_indices, cameras[0].hsize * cameras[0].vsize)
        rgb = np.empty((n, 3), dtype=np.float64)
        self._rtc(lib.rtc_render_shutter(scenes, cams, K, sh, sp, int(fuel), idx_p, 0, n, rgb.ctypes.data, stats), "rtc_render_shutter")
        return rgb

    def shutter_deal(self, hsize: int, n_poses: int, sampling: Sampling, shutter: Shutter, pixel_indices: Optional[np.ndarray] = None, first: int = 0,
                     n: Optional[int] = None, nw: Optional[NativeWorld] = None, device: int = 0):
        """include/rtc.h rtc_shutter_deal: the dealing alone for the pixels first .. first + n - 1 or the listed ones of a frame `hsize`
        wide.  Returns (order[n * side * side] of uint32: the sample ids pose-major, offsets[n_poses + 1] of uint64: the runs' starts).
        With a world the device kernels deal, without one the same rule is evaluated on the host (no GPU needed)."""
        lib = self._need("a shutter needs", "rtc_render_shutter", "rtc_shutter_deal")
        scene = self._scene(nw, device)
        if pixel_indices is None and n is None:
            raise ValueError("shutter_deal: give pixel_indices or n")
        n, idx_p, _keep = self._pixels(pixel_indices, n)
        sp, sh = SamplingC.of(sampling), ShutterC.of(shutter)
        order = np.empty(int(n) * sampling.samples, dtype=np.uint32)
        offsets = np.empty(max(0, int(n_poses)) + 1, dtype=np.uint64)
        self._rtc(lib.rtc_shutter_deal(scene, int(hsize), int(n_poses), sh, sp, idx_p, int(first), int(n), order.ctypes.data, offsets.ctypes.data), "rtc_shutter_deal")
        return order, offsets

    def scan_raw(self, values: np.ndarray, nw: Optional[NativeWorld] = None, device: int = 0):
        """include/rtc.h rtc_scan_raw (test infrastructure): (the exclusive prefix sums of `values` as a new uint64 array, their total),
        sums modulo 2^64.  With a world the device's scan kernels form them, without one a plain loop on the host (no GPU needed)."""
        lib = self._need("the scan hook needs", "rtc_scan_raw")
        scene = self._scene(nw, device)
        out = np.array(values, dtype=np.uint64, order="C", copy=True).reshape(-1)
        total = C.c_uint64(0)
        self._rtc(lib.rtc_scan_raw(scene, out.ctypes.data if out.size else None, out.size, C.byref(total)), "rtc_scan_raw")
        return out, int(total.value)

    def cull_probe(self, kind: int, records: np.ndarray, nw: Optional[NativeWorld] = None, device: int = 0) -> np.ndarray:
        """include/rtc.h rtc_cull_probe_raw (test infrastructure): one culling predicate of the ray kernels on `records` (one row of
        doubles each, the layout of RTC_CULL_* `kind`); returns one bool per record.  librtc_amd.so runs the probe kernel on the world's
        device and needs a world; the CPU emulator evaluates the same functions on the host and needs none."""
        lib = self._lib
        if not hasattr(lib, "rtc_cull_probe_raw"):
            raise RtwError("backend %r has no rtc_cull_probe_raw" % self.name)
        scene = self._scene(nw, device)
        rec = np.ascontiguousarray(records, dtype=np.float64)
        width = {0: 18, 1: 17, 2: 12, 3: 3, 4: 9}.get(int(kind))
        if rec.ndim != 2 or rec.shape[1] != width:
            raise ValueError("cull_probe: kind %r takes rows of %r doubles, got an array of shape %r" % (kind, width, rec.shape))
        n = rec.shape[0]
        out = np.zeros(n, dtype=np.uint8)
        self._rtc(lib.rtc_cull_probe_raw(scene, int(kind), rec.ctypes.data if n else None, n, out.ctypes.data if n else None), "rtc_cull_probe_raw")
        return out.astype(bool)

    def color_at(self, nw: NativeWorld, rays: np.ndarray, fuel: int = FUEL):
        """World::color_at for rays given as rows {ox,oy,oz,dx,dy,dz}.  Returns (rgb[n,3], hits[n])."""
        rays = np.ascontiguousarray(rays, dtype=np.float64).reshape(-1, 6)
        n = rays.shape[0]
        rgb = np.empty((n, 3), dtype=np.float64)
        hits = np.empty(n, dtype=HIT_DTYPE)
        self._check(self._lib.rtw_color_at(nw.handle, rays.ctypes.data, n, int(fuel), rgb.ctypes.data, hits.ctypes.data), "color_at")
        return rgb, hits
