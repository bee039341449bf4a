"""The C ABI of include/rtc.h and include/rtw.h as ctypes sees it: every struct once, every exported function's signature once.

``bind(lib)`` writes the signatures onto a freshly loaded library; nothing assigns ``argtypes`` or ``restype`` after that.
tests/test_cabi_mirror_cpu.py holds the structures and the table to the headers and to the library's dynamic symbols.

The convention of the table:
  * opaque handles (``rtc_scene*``, ``rtc_multi*``, every ``rtw_*`` handle) are ``c_void_p``; a pointer to a handle (``rtc_scene**``,
    ``rtw_element**``, an array of scenes) is ``POINTER(c_void_p)``;
  * a pointer to an ABI struct is ``POINTER(TheStructure)``: None, an instance, ``byref(x)`` and an array of the structure all pass;
    a raw address is cast by the caller.  Hit records (``rtc_hit*``, ``rtw_hit*``) are the exception: they live in numpy arrays of
    ``HIT_DTYPE`` and travel as addresses, so they are ``c_void_p`` like the pointers to scalars;
  * a pointer to scalars (``double*``, ``uint64_t*``, ``const int*``, ``double v[3]``, ``void*`` ...) is ``c_void_p``: a numpy
    ``.ctypes.data``, a torch ``data_ptr()``, a ctypes array and a ``byref`` all pass; C strings are ``c_char_p``;
  * scalars have their exact width.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from .scene import FILTER_KINDS, Adaptive, Filter, Sampling, Shutter

HIT_DTYPE = np.dtype([("t", "<f8"), ("prim", "<i4"), ("push_idx", "<i4")])   # rtc_hit / rtw_hit

i32, u32, u64, f64, vp = C.c_int32, C.c_uint32, C.c_uint64, C.c_double, C.c_void_p
P = C.POINTER


def _struct(name, *fields):
    return type(name, (C.Structure,), {"_fields_": list(fields)})


def _all(ctype, names):
    return [(n, ctype) for n in names.split()]


# ---- include/rtc.h ------------------------------------------------------------------------------------------------------------
RtcPrim = _struct("RtcPrim", *_all(i32, "geometry"), ("flags", u32), *_all(i32, "material xform data"))
RtcXform = _struct("RtcXform", ("transform_inv", f64 * 16), ("material_inv", f64 * 16))
RtcMaterial = _struct("RtcMaterial", *_all(f64, "ambient diffuse specular shininess reflective transparency refractive_index"), *_all(i32, "pattern _pad"))
RtcPatternNode = _struct("RtcPatternNode", *_all(i32, "tag kind noise_kind"), ("octaves", u32), *_all(i32, "left right"), ("scale", f64), ("color", f64 * 3),
                         ("transform_inv", f64 * 16))
RtcLight = _struct("RtcLight", ("intensity", f64 * 3), ("origin", f64 * 3))
RtcLightEx = _struct("RtcLightEx", ("kind", i32), *_all(u32, "usteps vsteps flags"), ("intensity", f64 * 3), ("corner", f64 * 3), ("uvec", f64 * 3), ("vvec", f64 * 3))
RtcUvPattern = _struct("RtcUvPattern", *_all(i32, "kind texture"), *_all(f64, "width height"), ("child", i32 * 5), ("_pad", i32))
RtcTexture = _struct("RtcTexture", *_all(u32, "width height"), ("rgb", vp))
RtcSceneExt = _struct("RtcSceneExt", ("n_lights", u32), ("lights", P(RtcLightEx)), ("n_uv_patterns", u32), ("uv_patterns", P(RtcUvPattern)), ("n_textures", u32),
                      ("textures", P(RtcTexture)))
RtcLightCone = _struct("RtcLightCone", *_all(u32, "light _pad"), ("axis", f64 * 3), *_all(f64, "cos_inner cos_outer"))
RtcBackground = _struct("RtcBackground", *_all(i32, "pattern projection"))
RtcBump = _struct("RtcBump", ("material", u32), ("kind", i32), *_all(u32, "octaves _pad"), *_all(f64, "amplitude frequency"))
RtcNode = _struct("RtcNode", *_all(i32, "kind ref skip _pad"), ("bbox_min", f64 * 3), ("bbox_max", f64 * 3))
RtcSceneDesc = _struct("RtcSceneDesc", ("n_nodes", u32), ("nodes", P(RtcNode)), ("n_prims", u32), ("prims", P(RtcPrim)), ("n_xforms", u32), ("xforms", P(RtcXform)),
                       ("n_limits", u32), ("limits", P(f64)), ("n_tris", u32), ("tri_p1e1e2", P(f64)), ("tri_normals", P(f64)),
                       ("n_materials", u32), ("materials", P(RtcMaterial)), ("n_pattern_nodes", u32), ("pattern_nodes", P(RtcPatternNode)),
                       ("n_lights", u32), ("lights", P(RtcLight)))
RtcCameraC = _struct("RtcCameraC", *_all(u64, "hsize vsize"), *_all(f64, "half_width half_height pixel_size"), ("transform_inv", f64 * 16))
RtcHit = _struct("RtcHit", ("t", f64), *_all(i32, "prim push_idx"))
RtcBackgroundInfo = _struct("RtcBackgroundInfo", *_all(i32, "has_background pattern projection plain_root trace_build trace_area trace_uv trace_spot wf_background_build _pad"))
RtcBumpInfo = _struct("RtcBumpInfo", ("has_bump", i32), ("n_bumps", u32), *_all(i32, "trace_build trace_area trace_uv trace_spot trace_bg wf_shade_build"))
RtcKernelInfo = _struct("RtcKernelInfo", *_all(i32, "variant n_kops n_kplanes n_kaux has_recs all_plain no_glass_mirror big_scene"), ("lds_bytes", u32),
                        *_all(i32, "trace_build wf_ts_build wf_shade_build0 wf_shade_build n_bvh_nodes n_recs n_mesh_tris has_mesh bvh_stack lds_refused"))


class RtcStatsC(C.Structure):
    _COUNTERS = ("pixels", "rays_primary", "rays_shadow", "rays_reflect", "rays_refract", "rays_container",
                 "accel_nodes", "group_tests", "tri_tests", "analytic_tests", "nan_ts")
    _fields_ = [(n, u64) for n in _COUNTERS] + [("kernel_ms", f64), ("n_launches", u32), ("_pad", u32)] + \
        _all(u64, "accel_nodes_kernarg analytic_tests_kernarg light_grid_cells group_tests_uniform")

    def as_dict(self):
        d = {n: int(getattr(self, n)) for n in self._COUNTERS + ("accel_nodes_kernarg", "analytic_tests_kernarg", "light_grid_cells", "group_tests_uniform")}
        d["kernel_ms"] = float(self.kernel_ms)
        d["n_launches"] = int(self.n_launches)
        d["unique_rays"] = d["rays_primary"] + d["rays_shadow"] + d["rays_reflect"] + d["rays_refract"]
        return d


class SamplingC(C.Structure):
    _fields_ = [("side", u32), ("flags", u32), ("seed", u64), ("lens_radius", f64), ("focal_distance", f64)]

    @staticmethod
    def of(s: Sampling) -> "SamplingC":
        return SamplingC(int(s.side), 1 if s.jitter else 0, int(s.seed), float(s.lens_radius), float(s.focal_distance))


class AdaptiveC(C.Structure):
    _fields_ = [("base", SamplingC), ("fine", SamplingC), ("threshold", f64), ("neighbours", u32), ("_pad", u32)]

    @staticmethod
    def of(a: Adaptive) -> "AdaptiveC":
        return AdaptiveC(SamplingC.of(a.base), SamplingC.of(a.fine), float(a.threshold), int(a.neighbours), 0)


class FilterC(C.Structure):
    _fields_ = [("kind", i32), ("_pad", u32), ("radius", f64), ("alpha", f64)]

    @staticmethod
    def of(f: Filter) -> "FilterC":
        return FilterC(FILTER_KINDS.index(f.kind), 0, float(f.radius), float(f.alpha))


class ShutterC(C.Structure):
    _fields_ = [("flags", u32), ("_pad", u32)]

    @staticmethod
    def of(s: Shutter) -> "ShutterC":
        return ShutterC(1 if s.hashed else 0, 0)


# ---- include/rtw.h ------------------------------------------------------------------------------------------------------------
MaterialC = _struct("MaterialC", *_all(f64, "ambient diffuse specular shininess reflective transparency refractive_index"), ("pattern", vp))
CameraC = _struct("CameraC", *_all(u64, "hsize vsize"), ("field_of_view", f64), ("transform", f64 * 16))
RtwHit = _struct("RtwHit", ("t", f64), *_all(i32, "prim push_idx"))
UvFaceC = _struct("UvFaceC", ("kind", C.c_int), *_all(f64, "width height"), ("texture", vp), ("child", vp * 5))

STRUCTS = {
    "rtc_prim": RtcPrim, "rtc_xform": RtcXform, "rtc_material": RtcMaterial, "rtc_pattern_node": RtcPatternNode, "rtc_light": RtcLight,
    "rtc_light_ex": RtcLightEx, "rtc_uv_pattern": RtcUvPattern, "rtc_texture": RtcTexture, "rtc_scene_ext": RtcSceneExt, "rtc_light_cone": RtcLightCone,
    "rtc_background": RtcBackground, "rtc_bump": RtcBump, "rtc_sampling": SamplingC, "rtc_adaptive": AdaptiveC, "rtc_filter": FilterC,
    "rtc_shutter": ShutterC, "rtc_node": RtcNode, "rtc_scene_desc": RtcSceneDesc, "rtc_camera": RtcCameraC, "rtc_hit": RtcHit, "rtc_stats": RtcStatsC,
    "rtc_background_info": RtcBackgroundInfo, "rtc_bump_info": RtcBumpInfo, "rtc_kernel_info": RtcKernelInfo,
    "rtw_material": MaterialC, "rtw_camera": CameraC, "rtw_hit": RtwHit, "rtw_uv_pattern": UvFaceC,
}

# ---- the signatures: name -> (restype, argtypes) ------------------------------------------------------------------------------
i, sz, s = C.c_int, C.c_size_t, C.c_char_p
PP = P(vp)
DESC, EXT, CAM, ST, SP = P(RtcSceneDesc), P(RtcSceneExt), P(RtcCameraC), P(RtcStatsC), P(SamplingC)
_CONES, _BG, _BUMPS = [P(RtcLightCone), u32], [P(RtcBackground)], [P(RtcBump), u32]
_CREATE = {"": [], "_ex": [P(RtcLightEx), u32], "_ext": [EXT], "_ext2": [EXT] + _CONES, "_ext3": [EXT] + _CONES + _BG, "_ext4": [EXT] + _CONES + _BG + _BUMPS}
_BANDS = [i32, u32, u32, u32, u32, vp, ST, i, i]   # fuel, band_rows, band_first, band_step, n_rows, rgb_dev, stats, count_stats, sync

SIGNATURES = {
    "rtc_last_error": (s, []),
    "rtc_device_count": (i, []),
    **{"rtc_scene_create" + level: (i, [DESC] + extra + [i, PP]) for level, extra in _CREATE.items()},
    **{"rtc_multi_create" + level: (i, [DESC] + extra + [vp, i, PP]) for level, extra in _CREATE.items()},
    "rtc_background_point": (i, [i32, vp, vp]),
    "rtc_background_colors": (i, [vp, vp, u64, vp]),
    "rtc_scene_background_info": (i, [vp, P(RtcBackgroundInfo)]),
    "rtc_bump_normal": (i, [P(RtcBump), vp, vp, vp, vp]),
    "rtc_bump_normals": (i, [vp, vp, vp, vp, u64, vp]),
    "rtc_scene_bump_info": (i, [vp, P(RtcBumpInfo)]),
    "rtc_spot_factor": (i, [P(RtcLightCone), vp, vp, vp]),
    "rtc_texture_sample": (i, [P(RtcTexture), i32, f64, f64, vp]),
    "rtc_scene_destroy": (None, [vp]),
    "rtc_scene_device_bytes": (u64, [vp]),
    "rtc_render": (i, [vp, CAM, i32, vp, u64, u64, vp, vp, ST]),
    "rtc_render_hit_digest": (i, [vp, CAM, i32, vp, u64, u64, vp]),
    "rtc_render_rgb8": (i, [vp, CAM, i32, vp, ST]),
    "rtc_render_rows_device": (i, [vp, CAM, i32, u32, u32, u32, vp, ST, i, i]),
    "rtc_render_bands_device": (i, [vp, CAM] + _BANDS),
    "rtc_band_rows_owned": (u64, [u64, u32, u32, u32]),
    "rtc_multi_destroy": (None, [vp]),
    "rtc_multi_device_count": (i, [vp]),
    "rtc_multi_set_band_rows": (i, [vp, u32]),
    "rtc_render_multi": (i, [vp, CAM, i32, vp, ST]),
    "rtc_render_multi_rgb8": (i, [vp, CAM, i32, vp, ST]),
    "rtc_render_multi_device": (i, [vp, CAM, i32, vp, i]),
    "rtc_multi_sync": (i, [vp]),
    "rtc_trace_rays": (i, [vp, vp, u64, i32, vp, vp, ST]),
    "rtc_render_sampled": (i, [vp, CAM, SP, i32, vp, u64, u64, vp, ST]),
    "rtc_render_sampled_rgb8": (i, [vp, CAM, SP, i32, vp, ST]),
    "rtc_render_sampled_bands_device": (i, [vp, CAM, SP] + _BANDS),
    "rtc_render_multi_sampled": (i, [vp, CAM, SP, i32, vp, ST]),
    "rtc_camera_rays": (i, [vp, CAM, SP, vp, u64, u64, vp]),
    "rtc_render_adaptive": (i, [vp, CAM, P(AdaptiveC), i32, vp, vp, vp, ST]),
    "rtc_render_adaptive_rgb8": (i, [vp, CAM, P(AdaptiveC), i32, vp, vp, vp, ST]),
    "rtc_contrast_pixels": (i, [vp, u64, u64, vp, f64, u32, vp, vp]),
    "rtc_render_filtered": (i, [vp, CAM, SP, P(FilterC), i32, u32, u32, vp, ST]),
    "rtc_render_filtered_rgb8": (i, [vp, CAM, SP, P(FilterC), i32, vp, ST]),
    "rtc_filter_frame": (i, [vp, u64, u64, SP, P(FilterC), vp, vp]),
    "rtc_render_shutter": (i, [PP, CAM, u32, P(ShutterC), SP, i32, vp, u64, u64, vp, ST]),
    "rtc_render_shutter_rgb8": (i, [PP, CAM, u32, P(ShutterC), SP, i32, vp, ST]),
    "rtc_shutter_deal": (i, [vp, u64, u32, P(ShutterC), SP, vp, u64, u64, vp, vp]),
    "rtc_shutter_draw_pose": (u32, [f64, u32]),
    "rtc_quantize_device": (i, [vp, vp, u64, vp, i]),
    "rtc_quantize": (i, [vp, vp, u64, vp]),
    "rtc_ppm": (u64, [u64, u64, vp, s, u64]),
    "rtc_scene_check": (i, [vp]),
    "rtc_scene_record": (i, [vp, i]),
    "rtc_scene_wait": (i, [vp, i]),
    "rtc_scene_elapsed_ms": (i, [vp, i, i, vp]),
    "rtc_scene_sync": (i, [vp]),
    "rtc_scene_accel_info": (None, [vp, vp, vp, vp, vp]),
    "rtc_scene_bvh_built_on_device": (i, [vp]),
    "rtc_bvh_build_raw": (i, [vp, u32, i32, u32, i32, vp, u32, vp, vp, u32, vp, u32, vp, vp, vp, vp]),
    "rtc_bvh_collapse_raw": (i, [vp, u32, i32, vp, vp]),
    "rtc_light_grid_build_raw": (i, [vp, vp, vp, vp, u32, vp, i32, i32, i32, vp, u32, vp, u32, vp]),
    "rtc_scan_raw": (i, [vp, vp, u64, vp]),
    "rtc_cull_probe_raw": (i, [vp, i32, vp, u64, vp]),
    "rtc_scene_wavefront_lds_bytes": (u32, [vp]),
    "rtc_scene_wavefront_ts_grid": (i, [vp, i32, vp, vp, vp, vp]),
    "rtc_scene_kernel_info": (i, [vp, i32, i32, P(RtcKernelInfo)]),
    "rtc_scene_path_info": (None, [vp, vp, vp, vp]),
    "rtw_last_error": (s, []),
    "rtw_backend": (s, []),
    "rtw_pattern_debug": (vp, []),
    "rtw_pattern_plain": (vp, [f64, f64, f64]),
    "rtw_pattern_jitter": (vp, [i, i, f64, u64, vp]),
    "rtw_pattern_mixture": (vp, [i, vp, vp, vp]),
    "rtw_pattern_release": (None, [vp]),
    "rtw_texture_create": (vp, [u32, u32, vp]),
    "rtw_texture_release": (None, [vp]),
    "rtw_pattern_uv": (vp, [i, vp, P(UvFaceC), sz]),
    "rtw_shape": (vp, [i, vp, P(MaterialC), i, vp, sz]),
    "rtw_composite": (vp, [vp, P(MaterialC), i, PP, sz]),
    "rtw_parse_obj": (vp, [s, vp, P(MaterialC), vp, vp]),
    "rtw_element_set_bump": (i, [vp, i32, u32, f64, f64]),
    "rtw_element_release": (None, [vp]),
    "rtw_world_create": (vp, []),
    "rtw_world_add_light": (i, [vp, vp, vp]),
    "rtw_world_add_area_light": (i, [vp, vp, vp, vp, u32, vp, u32, i]),
    "rtw_world_set_light_cone": (i, [vp, u32, vp, f64, f64]),
    "rtw_world_set_background": (i, [vp, vp, i32]),
    "rtw_world_add_element": (i, [vp, vp]),
    "rtw_world_primitive_count": (u64, [vp]),
    "rtw_world_release": (None, [vp]),
    "rtw_render": (i, [vp, P(CameraC), i, vp, u64, vp, vp]),
    "rtw_color_at": (i, [vp, vp, u64, i, vp, vp]),
    # exported by the product library, declared by no header (csrc/rtw_capi.cpp): the bridge from rtw_* handles to rtc.h
    "rtw_world_scene": (vp, [vp, i]),
    "rtw_make_camera": (i, [P(CameraC), CAM]),
    "rtw_world_flatten_counts": (i, [vp, vp]),
    "rtw_world_flatten_desc": (i, [vp, DESC]),
    # exported by the CPU emulator alone (tests/cpu_emu): the group gate's box test on (bbox_min .. bbox_max, ray origin .. direction)
    "rtc_emu_group_box_hit": (i, [vp, vp]),
}


def bind(lib):
    """Declare to ctypes every function of the table that `lib` exports (the CPU emulator and the oracle export subsets).  Once per
    loaded library; idempotent.  Returns `lib`."""
    for name, (res, args) in SIGNATURES.items():
        if hasattr(lib, name):
            fn = getattr(lib, name)
            fn.restype, fn.argtypes = res, list(args)
    return lib


def load(path):
    return bind(C.CDLL(path))
