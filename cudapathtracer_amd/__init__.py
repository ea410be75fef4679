"""cudapathtracer_amd -- MI355X-native (gfx950) re-authoring of CulDeVu/CUDAPathTracer's
per-pixel path-integration loop behind a C-ABI (include/pt/pt.h, libptamd.so).

Host surface (OBJ ingest, BVH build, camera, PPM) is C++ in csrc/host; the render path is
hand-written HIP in csrc/hip.  Python here is only orchestration over ctypes.
"""
from ._lib import (PT_FLAG_COUNT, PT_FLAG_NO_DEAD_PATH_SKIP, PT_FLAG_NO_PRIMARY_CACHE,  # noqa: F401
                   PT_FLAG_REFERENCE_TRAVERSAL, PT_FLAG_REFERENCE_BVH, PT_FLAG_TRI_COUNTS, PT_FLAG_JITTER, PT_FLAG_JITTER_TENT,
                   PT_INTEGRATOR_HEAD, PT_INTEGRATOR_UNIDIR, PtError, LIB_PATH, PT_E_INVALID, PT_E_IO, PT_E_SCENE,
                   PT_LIGHT_SPHERE, PT_ORDER_SCANLINE, PT_ORDER_MORTON, PT_FEATURE_EMISSIVE, PT_DENOISE_NO_DEMODULATE,
                   DenoiseParams, DenoiseGuidedParams, Feature, NoiseParams, NoiseSummary,
                   PT_SESSION_COUNTS, PT_SESSION_NOISE, PT_SESSION_NOISE_PER_PIXEL, View, TemporalParams,
                   PT_LIGHTMAP_NO_ALBEDO, LightmapParams)
from . import api  # noqa: F401
from . import rays  # noqa: F401  (ray sets for Renderer.render_rays)
from .api import (Accumulator, NoiseEstimate, noise_defaults, Group, Renderer, Scene, accum_file_info, session_file_info, camera_ray, make_camera, morton_i_to_pxl, morton_pxl_to_i,  # noqa: F401
                  tonemap_u8, write_ppm, write_ppm_codes, write_pfm, read_pfm, FEATURE, denoise_defaults, denoise_guided_defaults,
                  make_view, look_at, session_file_view, jitter_offset, project, temporal_defaults, Temporal)

__all__ = ["Scene", "Renderer", "Group", "Accumulator", "accum_file_info", "make_camera", "camera_ray", "morton_pxl_to_i", "morton_i_to_pxl", "write_ppm", "write_ppm_codes", "write_pfm", "read_pfm",
           "tonemap_u8", "PtError", "FEATURE", "Feature", "DenoiseParams", "denoise_defaults", "DenoiseGuidedParams", "denoise_guided_defaults", "NoiseEstimate", "noise_defaults", "NoiseParams",
           "NoiseSummary", "session_file_info", "PT_SESSION_COUNTS", "PT_SESSION_NOISE", "PT_SESSION_NOISE_PER_PIXEL", "View", "make_view", "look_at", "session_file_view", "jitter_offset",
           "PT_FLAG_JITTER", "PT_FLAG_JITTER_TENT", "project", "temporal_defaults", "Temporal", "TemporalParams", "rays",
           "PT_LIGHTMAP_NO_ALBEDO", "LightmapParams"]
