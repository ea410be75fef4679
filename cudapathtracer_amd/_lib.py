"""ctypes declarations for libptamd.so (include/pt/pt.h).  No compute happens in Python.

The library is built in-tree (``python __graft_entry__.py build`` or
``make -C cudapathtracer_amd/csrc``).  If it is missing this module raises immediately: there
is no Python or CPU fallback for the render path.
"""
from __future__ import annotations

import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
# PT_LIB selects an experiment build (tools/build_variants.sh); the default is the in-tree library
LIB_PATH = os.environ.get("PT_LIB") or os.path.join(_HERE, "libptamd.so")

PT_OK = 0
PT_E_INVALID, PT_E_IO, PT_E_SCENE, PT_E_BVH_DEPTH, PT_E_HIP, PT_E_NODEV, PT_E_OOM = -1, -2, -3, -4, -5, -6, -7
PT_INTEGRATOR_UNIDIR, PT_INTEGRATOR_HEAD = 0, 1
PT_FLAG_REFERENCE_TRAVERSAL = 0x1
PT_FLAG_NO_DEAD_PATH_SKIP = 0x2
PT_FLAG_NO_PRIMARY_CACHE = 0x4
PT_FLAG_COUNT = 0x8
PT_FLAG_REFERENCE_BVH = 0x10
PT_FLAG_TRI_COUNTS = 0x20
PT_FLAG_JITTER = 0x40        # sub-pixel jitter, box filter over the pixel footprint
PT_FLAG_JITTER_TENT = 0x80   # with PT_FLAG_JITTER: tent of half-width 1 pixel
PT_ORDER_SCANLINE, PT_ORDER_MORTON = 0, 1
PT_LIGHT_SPHERE = 0x80000000     # lights[] entry of an emissive sphere
ABI_VERSION = 6                 # PT_ABI_VERSION of include/pt/pt.h these bindings mirror
PT_BVH_LEAF_FLAG = 0x80000000


class Vec3(C.Structure):
    _fields_ = [("x", C.c_float), ("y", C.c_float), ("z", C.c_float)]


class Triangle(C.Structure):
    _fields_ = [("v0", C.c_int32), ("v1", C.c_int32), ("v2", C.c_int32), ("norm", Vec3), ("mat", C.c_int32)]


class Material(C.Structure):
    _fields_ = [("albedo", C.c_double * 3), ("emission", C.c_double * 3)]


class BvhNode(C.Structure):
    _fields_ = [("lo", Vec3), ("hi", Vec3), ("left", C.c_uint32), ("right", C.c_uint32)]


class Camera(C.Structure):
    _fields_ = [("pos", Vec3), ("dist_from_film", C.c_float), ("focal_length", C.c_float), ("radius", C.c_float),
                ("pxl_width", C.c_int32), ("pxl_height", C.c_int32)]


class View(C.Structure):   # pt_view, 44 B: the oriented camera's basis and film extent
    _fields_ = [("right", C.c_float * 3), ("up", C.c_float * 3), ("back", C.c_float * 3),
                ("film_w", C.c_float), ("film_h", C.c_float)]


class Sphere(C.Structure):   # sphere.h:7-12 (pt_sphere)
    _fields_ = [("pos", Vec3), ("rad", C.c_float), ("diffuse", C.c_double * 3), ("emission", C.c_double * 3)]


class SceneView(C.Structure):
    _fields_ = [("num_verts", C.c_uint32), ("num_tris", C.c_uint32), ("num_mats", C.c_uint32),
                ("num_lights", C.c_uint32), ("verts", C.POINTER(Vec3)), ("tris", C.POINTER(Triangle)),
                ("mats", C.POINTER(Material)), ("lights", C.POINTER(C.c_uint32)), ("total_light_area", C.c_float),
                ("bvh", C.POINTER(BvhNode)), ("bvh_size", C.c_uint32), ("bvh_depth", C.c_int32),
                ("spheres", C.POINTER(Sphere)), ("num_spheres", C.c_uint32)]


class Params(C.Structure):
    _fields_ = [("width", C.c_int32), ("height", C.c_int32), ("spp", C.c_int32), ("bounces", C.c_int32),
                ("integrator", C.c_int32), ("flags", C.c_uint32), ("seed", C.c_uint64),
                ("shard_index", C.c_int32), ("shard_count", C.c_int32), ("pixel_order", C.c_int32),
                ("tile_w", C.c_int32), ("tile_h", C.c_int32)]


class Stats(C.Structure):
    _fields_ = [("seconds", C.c_double), ("kernel_ms", C.c_double), ("samples", C.c_uint64),
                ("rays_traced", C.c_uint64), ("rays_reference", C.c_uint64), ("rays_nominal", C.c_uint64),
                ("node_tests", C.c_uint64), ("tri_tests", C.c_uint64), ("walk_lane_slots", C.c_uint64),
                ("leaf_steps", C.c_uint64), ("shade_lane_slots", C.c_uint64), ("accel_fallbacks", C.c_uint64),
                ("walk_cycles", C.c_uint64), ("shade_cycles", C.c_uint64), ("spill_entries", C.c_uint64),
                ("lds_node_tests", C.c_uint64), ("work_units", C.c_uint64), ("split_pixels", C.c_uint64)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


class RayClasses(C.Structure):   # pt_ray_classes, 32 B
    _fields_ = [("regular", C.c_uint64), ("irregular", C.c_uint64), ("invalid", C.c_uint64),
                ("first_invalid", C.c_uint32), ("pad", C.c_uint32)]


PT_FEATURE_EMISSIVE = 0x40000000   # pt_feature.prim bit: the hit material emits
PT_DENOISE_NO_DEMODULATE = 0x1


class Feature(C.Structure):   # pt_feature, 48 B
    _fields_ = [("albedo", C.c_float * 3), ("depth", C.c_float), ("normal", C.c_float * 3), ("prim", C.c_int32),
                ("position", C.c_float * 3), ("reserved", C.c_float)]


class DenoiseParams(C.Structure):
    _fields_ = [("iterations", C.c_int32), ("normal_power_log2", C.c_int32), ("sigma_depth", C.c_float),
                ("sigma_color", C.c_float), ("flags", C.c_uint32)]


class DenoiseGuidedParams(C.Structure):
    _fields_ = [("base", DenoiseParams), ("sigma_luma", C.c_float)]


class TemporalParams(C.Structure):   # pt_temporal_params, 16 B
    _fields_ = [("max_history", C.c_int32), ("normal_min", C.c_float), ("plane_tol", C.c_float), ("flags", C.c_uint32)]


PT_LIGHTMAP_NO_ALBEDO = 0x1   # pt_lightmap_params.flags: the lightmap value alone, not albedo times it


class LightmapParams(C.Structure):   # pt_lightmap_params, 16 B
    _fields_ = [("fill", C.c_float * 3), ("flags", C.c_uint32)]


class NoiseParams(C.Structure):
    _fields_ = [("tol", C.c_float), ("y_floor", C.c_float)]


class NoiseSummary(C.Structure):
    _fields_ = [("samples", C.c_int64), ("batches", C.c_int32), ("pixels", C.c_uint64), ("converged", C.c_uint64),
                ("hist", C.c_uint64 * 64)]

    def as_dict(self):
        return dict(samples=int(self.samples), batches=int(self.batches), pixels=int(self.pixels),
                    converged=int(self.converged), hist=[int(v) for v in self.hist])


class ConvergeParams(C.Structure):
    _fields_ = [("pass_spp", C.c_int32), ("max_samples", C.c_int32), ("min_batches", C.c_int32),
                ("quantile", C.c_float), ("noise", NoiseParams)]


class ConvergeResult(C.Structure):
    _fields_ = [("passes", C.c_int32), ("stopped_converged", C.c_int32), ("last", NoiseSummary)]


class AdaptiveResult(C.Structure):
    _fields_ = [("passes", C.c_int32), ("stopped_converged", C.c_int32), ("last", NoiseSummary),
                ("active", C.c_uint64), ("samples_total", C.c_uint64)]


PT_SESSION_COUNTS, PT_SESSION_NOISE, PT_SESSION_NOISE_PER_PIXEL = 0x1, 0x2, 0x4   # pt_session_info.flags


class SessionInfo(C.Structure):   # pt_session_info, 136 B
    _fields_ = [("params", Params), ("cam", Camera), ("samples", C.c_int64), ("scene_digest", C.c_uint64),
                ("flags", C.c_uint32), ("noise_batches", C.c_int32), ("noise_n0", C.c_int64), ("noise_W", C.c_double),
                ("frozen_pixels", C.c_uint64)]


assert C.sizeof(SessionInfo) == 136
assert C.sizeof(Feature) == 48 and C.sizeof(DenoiseGuidedParams) == 24
assert C.sizeof(NoiseSummary) == 32 + 64 * 8 and C.sizeof(ConvergeParams) == 24
assert C.sizeof(Vec3) == 12 and C.sizeof(Triangle) == 28 and C.sizeof(Material) == 48
assert C.sizeof(BvhNode) == 32 and C.sizeof(Camera) == 32 and C.sizeof(View) == 44

# symbol -> (restype, argtypes); the list IS the exported surface of include/pt/pt.h
SIGNATURES = {
    "pt_abi_version": (C.c_int, []),
    "pt_last_error": (C.c_char_p, []),
    "pt_scene_new": (C.c_void_p, []),
    "pt_scene_free": (None, [C.c_void_p]),
    "pt_scene_load_obj": (C.c_int, [C.c_void_p, C.c_char_p, C.c_char_p, Vec3, C.c_float, C.c_int]),
    "pt_scene_last_warning": (C.c_char_p, [C.c_void_p]),
    "pt_scene_build_bvh": (C.c_int, [C.c_void_p]),
    "pt_scene_add_sphere": (C.c_int, [C.c_void_p, C.POINTER(Sphere)]),
    "pt_scene_view": (C.c_int, [C.c_void_p, C.POINTER(SceneView)]),
    "pt_morton_pxl_to_i": (C.c_uint32, [C.c_uint32, C.c_uint32]),
    "pt_morton_i_to_pxl": (None, [C.c_uint32, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]),
    "pt_camera_ray": (None, [C.POINTER(Camera), C.c_uint32, C.c_int, C.c_float, C.c_float,
                             C.POINTER(Vec3), C.POINTER(Vec3)]),
    "pt_view_look_at": (C.c_int, [Vec3, Vec3, Vec3, C.POINTER(View)]),
    "pt_view_set_fov": (C.c_int, [C.POINTER(View), C.POINTER(Camera), C.c_float, C.c_int, C.c_int]),
    "pt_view_validate": (C.c_int, [C.POINTER(View)]),
    "pt_camera_ray_view": (None, [C.POINTER(Camera), C.POINTER(View), C.c_uint32, C.c_int, C.c_float, C.c_float,
                                  C.POINTER(Vec3), C.POINTER(Vec3)]),
    "pt_jitter_offset": (C.c_int, [C.c_uint32, C.c_float, C.c_float, C.POINTER(C.c_float), C.POINTER(C.c_float)]),
    "pt_camera_ray_jitter": (None, [C.POINTER(Camera), C.POINTER(View), C.c_uint32, C.c_float, C.c_float, C.c_int, C.c_float,
                                    C.c_float, C.POINTER(Vec3), C.POINTER(Vec3)]),
    "pt_write_ppm": (C.c_int, [C.c_char_p, C.c_void_p, C.c_int, C.c_int]),
    "pt_write_ppm_f64": (C.c_int, [C.c_char_p, C.c_void_p, C.c_int, C.c_int]),
    "pt_write_ppm_order": (C.c_int, [C.c_char_p, C.c_void_p, C.c_int, C.c_int, C.c_int]),
    "pt_tonemap_u8": (C.c_int, [C.c_double]),
    "pt_accel_digest": (C.c_int, [C.POINTER(SceneView), C.POINTER(C.c_uint64), C.POINTER(C.c_uint32),
                                  C.POINTER(C.c_int32)]),
    "pt_create": (C.c_void_p, [C.POINTER(SceneView), C.c_int, C.POINTER(C.c_int)]),
    "pt_render": (C.c_int, [C.c_void_p, C.POINTER(Params), C.POINTER(Camera), C.c_void_p, C.POINTER(Stats)]),
    "pt_render_device": (C.c_int, [C.c_void_p, C.POINTER(Params), C.POINTER(Camera), C.c_void_p, C.c_void_p,
                                   C.POINTER(Stats)]),
    "pt_render_device_async": (C.c_int, [C.c_void_p, C.POINTER(Params), C.POINTER(Camera), C.c_void_p, C.c_void_p]),
    "pt_render_wait": (C.c_int, [C.c_void_p, C.POINTER(Stats)]),
    "pt_render_view": (C.c_int, [C.c_void_p, C.POINTER(Params), C.POINTER(Camera), C.POINTER(View), C.c_void_p,
                                 C.POINTER(Stats)]),
    "pt_render_device_view": (C.c_int, [C.c_void_p, C.POINTER(Params), C.POINTER(Camera), C.POINTER(View), C.c_void_p,
                                        C.c_void_p, C.POINTER(Stats)]),
    "pt_render_device_view_async": (C.c_int, [C.c_void_p, C.POINTER(Params), C.POINTER(Camera), C.POINTER(View),
                                              C.c_void_p, C.c_void_p]),
    "pt_trace": (C.c_int, [C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32]),
    "pt_trace_counts": (C.c_int, [C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32,
                                  C.c_void_p, C.POINTER(C.c_uint64)]),
    "pt_tri_counts": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint32]),
    "pt_trace_device": (C.c_int, [C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p]),
    "pt_occluded_device": (C.c_int, [C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p]),
    "pt_occluded": (C.c_int, [C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32]),
    "pt_render_rays_device": (C.c_int, [C.c_void_p, C.POINTER(Params), C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(Stats)]),
    "pt_render_rays": (C.c_int, [C.c_void_p, C.POINTER(Params), C.c_void_p, C.c_void_p, C.POINTER(Stats)]),
    "pt_rays_classify_device": (C.c_int, [C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.POINTER(RayClasses)]),
    "pt_render_irradiance_device": (C.c_int, [C.c_void_p, C.POINTER(Params), C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(Stats)]),
    "pt_render_irradiance": (C.c_int, [C.c_void_p, C.POINTER(Params), C.c_void_p, C.c_void_p, C.POINTER(Stats)]),
    "pt_points_classify_device": (C.c_int, [C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.POINTER(RayClasses)]),
    "pt_tonemap_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    "pt_tonemap": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p]),
    "pt_write_ppm_codes": (C.c_int, [C.c_char_p, C.c_void_p, C.c_int, C.c_int]),
    "pt_write_pfm": (C.c_int, [C.c_char_p, C.c_void_p, C.c_int, C.c_int]),
    "pt_shard_pixels": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_uint32,
                                  C.POINTER(C.c_uint32)]),
    "pt_group_create": (C.c_void_p, [C.POINTER(C.c_void_p), C.c_int, C.POINTER(C.c_int)]),
    "pt_group_size": (C.c_int, [C.c_void_p]),
    "pt_render_group": (C.c_int, [C.c_void_p, C.POINTER(Params), C.POINTER(Camera), C.c_void_p, C.POINTER(Stats)]),
    "pt_render_group_view": (C.c_int, [C.c_void_p, C.POINTER(Params), C.POINTER(Camera), C.POINTER(View), C.c_void_p,
                                       C.POINTER(Stats)]),
    "pt_render_multi_view": (C.c_int, [C.POINTER(C.c_void_p), C.c_int, C.POINTER(Params), C.POINTER(Camera),
                                       C.POINTER(View), C.c_void_p, C.POINTER(Stats)]),
    "pt_group_destroy": (None, [C.c_void_p]),
    "pt_render_multi": (C.c_int, [C.POINTER(C.c_void_p), C.c_int, C.POINTER(Params), C.POINTER(Camera), C.c_void_p,
                                  C.POINTER(Stats)]),
    "pt_accum_create": (C.c_void_p, [C.c_void_p, C.POINTER(Params), C.POINTER(Camera), C.POINTER(C.c_int)]),
    "pt_accum_create_view": (C.c_void_p, [C.c_void_p, C.POINTER(Params), C.POINTER(Camera), C.POINTER(View),
                                          C.POINTER(C.c_int)]),
    "pt_accum_view": (C.c_int, [C.c_void_p, C.POINTER(View), C.POINTER(C.c_int)]),
    "pt_accum_create_rays_device": (C.c_void_p, [C.c_void_p, C.POINTER(Params), C.c_void_p, C.c_void_p, C.POINTER(C.c_int)]),
    "pt_accum_create_rays": (C.c_void_p, [C.c_void_p, C.POINTER(Params), C.c_void_p, C.POINTER(C.c_int)]),
    "pt_accum_has_rays": (C.c_int, [C.c_void_p]),
    "pt_accum_create_points_device": (C.c_void_p, [C.c_void_p, C.POINTER(Params), C.c_void_p, C.c_void_p, C.POINTER(C.c_int)]),
    "pt_accum_create_points": (C.c_void_p, [C.c_void_p, C.POINTER(Params), C.c_void_p, C.POINTER(C.c_int)]),
    "pt_accum_has_points": (C.c_int, [C.c_void_p]),
    "pt_render_features_rays_device": (C.c_int, [C.c_void_p, C.POINTER(Params), C.c_void_p, C.c_void_p, C.c_void_p]),
    "pt_render_features_rays": (C.c_int, [C.c_void_p, C.POINTER(Params), C.c_void_p, C.c_void_p]),
    "pt_accum_add": (C.c_int, [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.POINTER(Stats)]),
    "pt_accum_samples": (C.c_int64, [C.c_void_p]),
    "pt_accum_read": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p]),
    "pt_accum_save": (C.c_int, [C.c_void_p, C.c_char_p]),
    "pt_accum_load": (C.c_void_p, [C.c_void_p, C.c_char_p, C.POINTER(C.c_int)]),
    "pt_accum_file_info": (C.c_int, [C.c_char_p, C.POINTER(Params), C.POINTER(Camera), C.POINTER(C.c_int64),
                                     C.POINTER(C.c_uint64)]),
    "pt_accum_destroy": (None, [C.c_void_p]),
    "pt_noise_defaults": (None, [C.POINTER(NoiseParams)]),
    "pt_noise_create": (C.c_void_p, [C.c_void_p, C.POINTER(C.c_int)]),
    "pt_noise_update": (C.c_int, [C.c_void_p, C.POINTER(NoiseParams), C.c_void_p, C.POINTER(NoiseSummary)]),
    "pt_noise_read": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p]),
    "pt_noise_map": (C.c_int, [C.c_void_p, C.POINTER(NoiseParams), C.c_void_p]),
    "pt_noise_map_device": (C.c_int, [C.c_void_p, C.POINTER(NoiseParams), C.c_void_p, C.c_void_p]),
    "pt_noise_variance": (C.c_int, [C.c_void_p, C.c_void_p]),
    "pt_noise_variance_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p]),
    "pt_noise_destroy": (None, [C.c_void_p]),
    "pt_accum_add_until": (C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(ConvergeParams), C.c_void_p, C.c_void_p,
                                     C.POINTER(ConvergeResult)]),
    "pt_accum_freeze": (C.c_int, [C.c_void_p, C.c_void_p]),
    "pt_accum_counts": (C.c_int, [C.c_void_p, C.c_void_p]),
    "pt_accum_active": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint32, C.POINTER(C.c_uint64)]),
    "pt_noise_freeze": (C.c_int, [C.c_void_p, C.POINTER(NoiseParams), C.c_void_p, C.POINTER(C.c_uint64),
                                  C.POINTER(C.c_uint64)]),
    "pt_accum_add_adaptive": (C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(ConvergeParams), C.c_void_p, C.c_void_p,
                                        C.POINTER(AdaptiveResult)]),
    "pt_session_save": (C.c_int, [C.c_void_p, C.c_void_p, C.c_char_p]),
    "pt_session_load": (C.c_int, [C.c_void_p, C.c_char_p, C.POINTER(C.c_void_p), C.POINTER(C.c_void_p),
                                  C.POINTER(C.c_int)]),
    "pt_session_file_info": (C.c_int, [C.c_char_p, C.POINTER(SessionInfo)]),
    "pt_session_file_view": (C.c_int, [C.c_char_p, C.POINTER(View), C.POINTER(C.c_int)]),
    "pt_denoise_defaults": (None, [C.POINTER(DenoiseParams)]),
    "pt_render_features_view_device": (C.c_int, [C.c_void_p, C.POINTER(Params), C.POINTER(Camera), C.POINTER(View),
                                                 C.c_void_p, C.c_void_p]),
    "pt_render_features_view": (C.c_int, [C.c_void_p, C.POINTER(Params), C.POINTER(Camera), C.POINTER(View), C.c_void_p]),
    "pt_render_features_device": (C.c_int, [C.c_void_p, C.POINTER(Params), C.POINTER(Camera), C.c_void_p, C.c_void_p]),
    "pt_render_features": (C.c_int, [C.c_void_p, C.POINTER(Params), C.POINTER(Camera), C.c_void_p]),
    "pt_denoise_device": (C.c_int, [C.c_void_p, C.POINTER(DenoiseParams), C.c_int, C.c_int, C.c_int, C.c_void_p,
                                    C.c_void_p, C.c_void_p, C.c_void_p]),
    "pt_denoise": (C.c_int, [C.c_void_p, C.POINTER(DenoiseParams), C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p,
                             C.c_void_p]),
    "pt_denoise_guided_defaults": (None, [C.POINTER(DenoiseGuidedParams)]),
    "pt_denoise_guided_device": (C.c_int, [C.c_void_p, C.POINTER(DenoiseGuidedParams), C.c_int, C.c_int, C.c_int, C.c_void_p,
                                           C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "pt_denoise_guided": (C.c_int, [C.c_void_p, C.POINTER(DenoiseGuidedParams), C.c_int, C.c_int, C.c_int, C.c_void_p,
                                    C.c_void_p, C.c_void_p, C.c_void_p]),
    "pt_project_view": (C.c_int, [C.POINTER(Camera), C.POINTER(View), Vec3, C.POINTER(C.c_float), C.POINTER(C.c_float)]),
    "pt_temporal_defaults": (None, [C.POINTER(TemporalParams)]),
    "pt_temporal_create": (C.c_void_p, [C.c_void_p, C.POINTER(TemporalParams), C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int)]),
    "pt_temporal_push_device": (C.c_int, [C.c_void_p, C.POINTER(Camera), C.POINTER(View), C.c_uint32, C.c_void_p, C.c_void_p,
                                          C.c_void_p, C.c_void_p, C.c_void_p]),
    "pt_temporal_push": (C.c_int, [C.c_void_p, C.POINTER(Camera), C.POINTER(View), C.c_uint32, C.c_void_p, C.c_void_p,
                                   C.c_void_p, C.c_void_p]),
    "pt_temporal_length": (C.c_int, [C.c_void_p, C.c_void_p]),
    "pt_temporal_frames": (C.c_int, [C.c_void_p]),
    "pt_temporal_reset": (C.c_int, [C.c_void_p]),
    "pt_temporal_destroy": (None, [C.c_void_p]),
    "pt_lightmap_dilate_device": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p,
                                            C.c_void_p, C.c_void_p]),
    "pt_lightmap_dilate": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "pt_lightmap_shade_device": (C.c_int, [C.c_void_p, C.POINTER(LightmapParams), C.c_uint32, C.c_void_p, C.c_void_p,
                                           C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    "pt_lightmap_shade": (C.c_int, [C.c_void_p, C.POINTER(LightmapParams), C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p,
                                    C.c_int, C.c_int, C.c_void_p]),
    "pt_destroy": (None, [C.c_void_p]),
}

_lib = None


def _torch_runtime_first():
    """One process, two HIP runtimes: PyTorch's ROCm wheel bundles its own (torch/lib/libamdhip64.so, loaded by path),
    libptamd.so links the system's (libamdhip64.so.7).  With this library's runtime up first, PyTorch then finds no
    device ("no ROCm-capable device is detected", profiles/r06_async_dbg); with PyTorch's first, both work (every suite
    and bench run).  So when PyTorch is importable and sees a GPU, its runtime is initialised before the library is
    loaded (PT_NO_TORCH_FIRST=1 skips this; the C-ABI itself never needs PyTorch)."""
    if os.environ.get("PT_NO_TORCH_FIRST"):
        return
    try:
        import torch
    except ImportError:
        return
    if torch.cuda.is_available():
        torch.cuda.init()


def lib():
    """Load libptamd.so once; raise loudly if it has not been built."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(
                "libptamd.so not found at %s: build it with `python __graft_entry__.py build` "
                "(there is no fallback render path)" % LIB_PATH)
        _torch_runtime_first()
        handle = C.CDLL(LIB_PATH)
        for name, (res, args) in SIGNATURES.items():
            fn = getattr(handle, name)
            fn.restype = res
            fn.argtypes = args
        if handle.pt_abi_version() != ABI_VERSION:
            raise RuntimeError("libptamd.so ABI %d, bindings expect %d: rebuild it" % (handle.pt_abi_version(), ABI_VERSION))
        _lib = handle
    return _lib


class PtError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__("pt error %d: %s" % (code, msg))
        self.code = code


def check(rc):
    if rc != PT_OK:
        raise PtError(rc, (lib().pt_last_error() or b"").decode(errors="replace"))
    return rc
