"""ctypes mirror of include/rt_hip.h (the C ABI of librt_hip.so).

Plain data types only: these structures are the drop-in boundary's argument types, shared by the
product wrapper (`cudaraytracer_amd.renderer`) and by the tests that feed the same inputs to the oracle.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

# enums (Hittable.cuh:30-38, Material.cuh:6-12, Texture.cuh:6-10)
RT_SPHERE, RT_XYRECT, RT_XZRECT, RT_YZRECT = 0, 1, 2, 3
RT_LAMBERTIAN, RT_METAL, RT_DIELECTRIC, RT_DIFFUSELIGHT = 0, 1, 2, 3
RT_CONSTANT, RT_CHECKER, RT_IMAGE = 0, 1, 2

RT_FLAG_FAITHFUL_GRID = 1 << 0
RT_FLAG_NO_STATE_WRITEBACK = 1 << 1
RT_FLAG_ACCUMULATE = 1 << 2
RT_FLAG_RIUS_LEFT_TO_RIGHT = 1 << 3
RT_FLAG_COUNT_TESTS = 1 << 4
RT_FLAG_RNG_PHILOX = 1 << 5
RT_FLAG_STATE_SOA = 1 << 6
RT_FLAG_ACCUMULATE_RESET = 1 << 7
RT_CAMERA_JITTER_PHILOX = 1 << 0
# rt_radiance_args.flags, rt_adaptive_samples_args.flags, rt_temporal_gradient_args.flags: next-event estimation on the
# scene's light rectangles
RT_RADIANCE_DIRECT_LIGHT = 1 << 8
RT_DENOISE_DEMODULATE = 1 << 0
RT_DENOISE_COLOR_IS_SUM = 1 << 1
RT_TEMPORAL_COLOR_IS_SUM = 1 << 0
RT_TEMPORAL_RESET = 1 << 1
# RT_ABI_VERSION; 9: rt_scene_motion, rt_temporal_dynamic, rt_scene_edit; 10: rt_tile_entries_host;
# 11: RT_TUNE_CAMERA_RESOLVE; 12: RT_TUNE_PATH_END_STEP; 13: rt_temporal_moments, rt_denoise_variance,
# rt_denoise_variance_scratch_bytes; 14: rt_query_rays, 32-bit references in rt_gbuffer and rt_trace_rays
# (rt_set_bounce_entries, rt_bounce_entries_host, rt_bounce_entry_cells, rt_occluded_rays, rt_camera_rays,
# rt_radiance_rays, rt_set_bounce_classes, rt_bounce_class_entries_host, rt_adaptive_select,
# rt_adaptive_select_scratch_bytes, rt_adaptive_samples, rt_temporal_gradient, rt_history_adapt,
# RT_RADIANCE_DIRECT_LIGHT and rt_scene_lights_host were added without a new number: no layout changed)
ABI_VERSION = 14
# entries (o.x, o.y, o.z, s) of the per-hittable motion table rt_scene_motion writes and rt_temporal_dynamic reads
MOTION_NO_HISTORY = (0.0, 0.0, 0.0, 0.0)
MOTION_IDENTITY = (0.0, 0.0, 0.0, 1.0)
COUNTERS_WORDS = 24  # RT_COUNTERS_WORDS: the counters buffer with RT_FLAG_COUNT_TESTS
PHILOX_MAX_SPP = 16384  # RT_PHILOX_MAX_SPP
# rt_set_tuning keys (rt_tuning_key in include/rt_hip.h)
RT_TUNE_REGEN_THRESHOLD, RT_TUNE_LEAF_MAX, RT_TUNE_PERSISTENT_WAVES, RT_TUNE_SAH_TRAVERSAL = 0, 1, 2, 3
RT_TUNE_LDS_PAD, RT_TUNE_ADAPTIVE_ORDER, RT_TUNE_TEXEL_LAYOUT, RT_TUNE_QUEUE_CHUNK = 4, 5, 6, 7
RT_TUNE_QUEUE_STRIDE, RT_TUNE_REGEN_LIVE_FRAC, RT_TUNE_LEAF_BREAK, RT_TUNE_RIUS_TRIPS = 8, 9, 10, 11
RT_TUNE_FLAT_MAX = 12
RT_TUNE_QUEUE_PREFETCH = 13
RT_TUNE_QUEUE_GUIDE = 14
RT_TUNE_QUEUE_MIN_CHUNK = 15
RT_TUNE_RIUS_TRIPS_PERSISTENT = 16
RT_TUNE_PREFETCH_STOP = 17
RT_TUNE_PERSISTENT_GROUP = 18  # persistent flat kernel: 16-wave workgroups with static tile shares (1) or not (0)
RT_TUNE_GROUP_ORDER = 20  # ... the shares' tiles interleaved (0) or in golden-ratio order (1)
RT_TUNE_QUEUE_RESET = 21  # 1 = rt_render memsets the persistent queue slot per launch
RT_TUNE_GROUP_CHUNK = 22  # ... positions per chunk of the workgroup chunk queue (group mode 2)
RT_TUNE_GROUP_LINGER_US = 23  # ... a finished workgroup waits this long (us) for the grid's others before exiting
RT_TUNE_GROUP_WAVES = 24  # ... waves per workgroup of the persistent flat kernel's group builds (4/8/12/16)
RT_TUNE_TILE_ENTRIES = 25  # v3: camera rays start at their tile's candidate leaves (1) or at the root (0)
# v3: a shading pass resolves the next camera rays of its paths that missed by a scan of the tile's candidates (1;
# 2..32: with that primitive cap) or leaves them to the leaf chain (0)
RT_TUNE_CAMERA_RESOLVE = 26
# v3: where that scan applies, every path end and the pixel's first camera ray go through it (1) or only misses do (0)
RT_TUNE_PATH_END_STEP = 27
RT_TUNE_GROUP_TAIL = 19 # ... permille of the tiles left to the per-wave queue behind the shares

STATUS = {
    0: "RT_OK",
    -1: "RT_ERR_INVALID_ARGUMENT",
    -2: "RT_ERR_INVALID_SCENE",
    -3: "RT_ERR_OUT_OF_MEMORY",
    -4: "RT_ERR_DEVICE",
    -5: "RT_ERR_LAUNCH",
    -6: "RT_ERR_UNSUPPORTED",
}

F3 = C.c_float * 3


class TextureDesc(C.Structure):
    _fields_ = [("type", C.c_int32), ("image", C.c_int32), ("color", F3), ("color2", F3)]


class MaterialDesc(C.Structure):
    _fields_ = [
        ("type", C.c_int32),
        ("fuzz", C.c_float),
        ("ir", C.c_float),
        ("light_intensity", C.c_int32),
        ("albedo", TextureDesc),
    ]


class HittableDesc(C.Structure):
    _fields_ = [
        ("type", C.c_int32),
        ("is_active", C.c_int32),
        ("center", F3),
        ("radius", C.c_float),
        ("width", C.c_float),
        ("height", C.c_float),
        ("material", C.c_int32),
        ("reserved", C.c_int32),
    ]


class ImageDesc(C.Structure):
    _fields_ = [("data", C.c_void_p), ("width", C.c_int32), ("height", C.c_int32)]


class SceneDesc(C.Structure):
    _fields_ = [
        ("hittables", C.POINTER(HittableDesc)),
        ("num_hittables", C.c_uint32),
        ("materials", C.POINTER(MaterialDesc)),
        ("num_materials", C.c_uint32),
        ("images", C.POINTER(ImageDesc)),
        ("num_images", C.c_uint32),
    ]


class InputStruct(C.Structure):
    """InputStruct (Utils/SharedStructs.h:3-24), 72 bytes."""

    _fields_ = [
        ("origin", F3),
        ("orientation", F3),
        ("up", F3),
        ("far_plane", C.c_float),
        ("near_plane", C.c_float),
        ("fov", C.c_float),
        ("background_start", F3),
        ("background_end", F3),
    ]


class CurandState(C.Structure):
    """curandStateXORWOW layout, 48 bytes."""

    _fields_ = [
        ("d", C.c_uint32),
        ("v", C.c_uint32 * 5),
        ("boxmuller_flag", C.c_int32),
        ("boxmuller_flag_double", C.c_int32),
        ("boxmuller_extra", C.c_float),
        ("pad_", C.c_uint32),
        ("boxmuller_extra_double", C.c_double),
    ]


class Dim3(C.Structure):
    _fields_ = [("x", C.c_uint32), ("y", C.c_uint32), ("z", C.c_uint32)]


class Tiling(C.Structure):
    _fields_ = [
        ("band_rows", C.c_uint32),
        ("num_ranks", C.c_uint32),
        ("rank", C.c_uint32),
        ("local_rows", C.c_uint32),
    ]


class RenderArgs(C.Structure):
    _fields_ = [
        ("pos", C.c_void_p),
        ("radiance", C.c_void_p),
        ("accum", C.c_void_p),
        ("state", C.c_void_p),
        ("counters", C.c_void_p),
        ("width", C.c_uint32),
        ("height", C.c_uint32),
        ("samples_per_pixel", C.c_uint32),
        ("max_depth", C.c_uint32),
        ("flags", C.c_uint32),
        ("reserved", C.c_uint32),
        ("tiling", Tiling),
        ("inputs", InputStruct),
        ("rng_seed", C.c_uint64),
        ("rng_frame", C.c_uint32),
        ("reserved2", C.c_uint32),
    ]


class GBufferArgs(C.Structure):
    _fields_ = [
        ("normal_depth", C.c_void_p),
        ("albedo", C.c_void_p),
        ("prim_id", C.c_void_p),
        ("width", C.c_uint32),
        ("height", C.c_uint32),
        ("reserved", C.c_uint32 * 2),
        ("tiling", Tiling),
        ("inputs", InputStruct),
    ]


class QueryArgs(C.Structure):  # rt_query_args
    _fields_ = [
        ("rays", C.c_void_p),
        ("normal_depth", C.c_void_p),
        ("albedo", C.c_void_p),
        ("prim_id", C.c_void_p),
        ("uv", C.c_void_p),
        ("material", C.c_void_p),
        ("hits", C.c_void_p),
        ("n", C.c_uint32),
        ("rays_per_lane", C.c_uint32),
        ("flags", C.c_uint32),
        ("reserved", C.c_uint32),
    ]


class OcclusionArgs(C.Structure):  # rt_occlusion_args
    _fields_ = [
        ("rays", C.c_void_p),
        ("occluded", C.c_void_p),
        ("blocker", C.c_void_p),
        ("counters", C.c_void_p),
        ("n", C.c_uint32),
        ("rays_per_lane", C.c_uint32),
        ("count_tests", C.c_uint32),
        ("flags", C.c_uint32),
        ("reserved", C.c_uint32 * 2),
    ]


class CameraRaysArgs(C.Structure):
    """rt_camera_rays_args, 160 bytes."""

    _fields_ = [
        ("rays", C.c_void_p),
        ("pixels", C.c_void_p),
        ("pixel_index", C.c_void_p),
        ("n", C.c_uint32),
        ("width", C.c_uint32),
        ("height", C.c_uint32),
        ("flags", C.c_uint32),
        ("tiling", Tiling),
        ("inputs", InputStruct),
        ("xi1", C.c_float),
        ("xi2", C.c_float),
        ("rng_seed", C.c_uint64),
        ("rng_frame", C.c_uint32),
        ("sample", C.c_uint32),
        ("reserved", C.c_uint32 * 2),
    ]


class RadianceArgs(C.Structure):
    """rt_radiance_args, 120 bytes."""

    _fields_ = [
        ("rays", C.c_void_p),
        ("stream_ids", C.c_void_p),
        ("sum", C.c_void_p),
        ("mean", C.c_void_p),
        ("counters", C.c_void_p),
        ("n", C.c_uint32),
        ("rays_per_lane", C.c_uint32),
        ("samples_per_ray", C.c_uint32),
        ("sample_base", C.c_uint32),
        ("max_depth", C.c_uint32),
        ("count_tests", C.c_uint32),
        ("flags", C.c_uint32),
        ("stream_base", C.c_uint32),
        ("rng_seed", C.c_uint64),
        ("rng_frame", C.c_uint32),
        ("background_start", F3),
        ("background_end", F3),
        ("reserved", C.c_uint32 * 3),
    ]


class AdaptiveSelectArgs(C.Structure):
    """rt_adaptive_select_args, 120 bytes."""

    _fields_ = [
        ("history", C.c_void_p),
        ("moments", C.c_void_p),
        ("prim_id", C.c_void_p),
        ("pixels", C.c_void_p),
        ("samples", C.c_void_p),
        ("count", C.c_void_p),
        ("scratch", C.c_void_p),
        ("width", C.c_uint32),
        ("height", C.c_uint32),
        ("capacity", C.c_uint32),
        ("max_samples", C.c_uint32),
        ("min_history", C.c_uint32),
        ("tau", C.c_float),
        ("lum_floor", C.c_float),
        ("pixels_per_lane", C.c_uint32),
        ("flags", C.c_uint32),
        ("reserved", C.c_uint32 * 3),
        ("tiling", Tiling),
    ]


class AdaptiveSamplesArgs(C.Structure):
    """rt_adaptive_samples_args, 192 bytes."""

    _fields_ = [
        ("pixels", C.c_void_p),
        ("samples", C.c_void_p),
        ("count", C.c_void_p),
        ("history", C.c_void_p),
        ("moments", C.c_void_p),
        ("accum", C.c_void_p),
        ("counters", C.c_void_p),
        ("capacity", C.c_uint32),
        ("width", C.c_uint32),
        ("height", C.c_uint32),
        ("samples_per_pixel", C.c_uint32),
        ("max_samples", C.c_uint32),
        ("sample_base", C.c_uint32),
        ("max_depth", C.c_uint32),
        ("max_history", C.c_uint32),
        ("rays_per_lane", C.c_uint32),
        ("count_tests", C.c_uint32),
        ("flags", C.c_uint32),
        ("rng_frame", C.c_uint32),
        ("rng_seed", C.c_uint64),
        ("inputs", InputStruct),
        ("reserved", C.c_uint32 * 2),
    ]


class TemporalGradientArgs(C.Structure):
    """rt_temporal_gradient_args, 192 bytes."""

    _fields_ = [
        ("prev_color", C.c_void_p),
        ("gradient", C.c_void_p),
        ("resample", C.c_void_p),
        ("pixel", C.c_void_p),
        ("counters", C.c_void_p),
        ("rng_seed", C.c_uint64),
        ("width", C.c_uint32),
        ("height", C.c_uint32),
        ("stride", C.c_uint32),
        ("offset_x", C.c_uint32),
        ("offset_y", C.c_uint32),
        ("samples_per_pixel", C.c_uint32),
        ("max_depth", C.c_uint32),
        ("rays_per_lane", C.c_uint32),
        ("count_tests", C.c_uint32),
        ("flags", C.c_uint32),
        ("rng_frame", C.c_uint32),
        ("reserved", C.c_uint32 * 3),
        ("tiling", Tiling),
        ("inputs", InputStruct),
    ]


class HistoryAdaptArgs(C.Structure):
    """rt_history_adapt_args, 72 bytes."""

    _fields_ = [
        ("gradient", C.c_void_p),
        ("history", C.c_void_p),
        ("width", C.c_uint32),
        ("height", C.c_uint32),
        ("stride", C.c_uint32),
        ("radius", C.c_uint32),
        ("power", C.c_uint32),
        ("gain", C.c_float),
        ("lum_floor", C.c_float),
        ("flags", C.c_uint32),
        ("tiling", Tiling),
        ("reserved", C.c_uint32 * 2),
    ]


class DenoiseArgs(C.Structure):
    _fields_ = [
        ("color", C.c_void_p),
        ("normal_depth", C.c_void_p),
        ("albedo", C.c_void_p),
        ("prim_id", C.c_void_p),
        ("out_color", C.c_void_p),
        ("pos", C.c_void_p),
        ("scratch", C.c_void_p),
        ("width", C.c_uint32),
        ("height", C.c_uint32),
        ("iterations", C.c_uint32),
        ("flags", C.c_uint32),
        ("sigma_c", C.c_float),
        ("sigma_n", C.c_float),
        ("sigma_z", C.c_float),
        ("reserved", C.c_uint32),
        ("tiling", Tiling),
    ]


class DenoiseVarianceArgs(C.Structure):
    """rt_denoise_variance_args, 112 bytes."""

    _fields_ = [
        ("color", C.c_void_p),
        ("moments", C.c_void_p),
        ("normal_depth", C.c_void_p),
        ("prim_id", C.c_void_p),
        ("out_color", C.c_void_p),
        ("pos", C.c_void_p),
        ("scratch", C.c_void_p),
        ("width", C.c_uint32),
        ("height", C.c_uint32),
        ("iterations", C.c_uint32),
        ("flags", C.c_uint32),
        ("sigma_l", C.c_float),
        ("sigma_n", C.c_float),
        ("sigma_z", C.c_float),
        ("min_history", C.c_uint32),
        ("reserved", C.c_uint32 * 2),
        ("tiling", Tiling),
    ]


class TemporalArgs(C.Structure):
    _fields_ = [
        ("color", C.c_void_p),
        ("normal_depth", C.c_void_p),
        ("prim_id", C.c_void_p),
        ("prev_history", C.c_void_p),
        ("prev_normal_depth", C.c_void_p),
        ("prev_prim_id", C.c_void_p),
        ("history", C.c_void_p),
        ("motion", C.c_void_p),
        ("pos", C.c_void_p),
        ("width", C.c_uint32),
        ("height", C.c_uint32),
        ("flags", C.c_uint32),
        ("max_history", C.c_uint32),
        ("depth_tol", C.c_float),
        ("normal_tol", C.c_float),
        ("reserved", C.c_uint32 * 2),
        ("tiling", Tiling),
        ("inputs", InputStruct),
        ("prev_inputs", InputStruct),
    ]


class TiledDesc(C.Structure):
    _fields_ = [("devices", C.POINTER(C.c_int)), ("num_ranks", C.c_uint32), ("band_rows", C.c_uint32),
                ("width", C.c_uint32), ("height", C.c_uint32), ("flags", C.c_uint32), ("reserved", C.c_uint32),
                ("seed", C.c_uint64)]


class TiledFrame(C.Structure):
    _fields_ = [("pos", C.c_void_p), ("samples_per_pixel", C.c_uint32), ("max_depth", C.c_uint32),
                ("flags", C.c_uint32), ("rng_frame", C.c_uint32), ("rng_frame_set", C.c_uint32),
                ("reserved", C.c_uint32), ("inputs", InputStruct)]


class TiledTiming(C.Structure):
    _fields_ = [("render_ms", C.c_float), ("gather_ms", C.c_float), ("total_ms", C.c_float), ("reserved", C.c_uint32),
                ("rays", C.c_uint64)]


class SceneInfo(C.Structure):
    _fields_ = [
        ("num_primitives", C.c_uint32),
        ("num_nodes", C.c_uint32),
        ("num_materials", C.c_uint32),
        ("bvh_depth", C.c_uint32),
        ("device_bytes", C.c_uint64),
    ]


class HostTablesInfo(C.Structure):
    _fields_ = [("num_nodes", C.c_uint32), ("num_prims", C.c_uint32), ("num_materials", C.c_uint32),
                ("depth", C.c_uint32)]


class BounceEntriesInfo(C.Structure):
    _fields_ = [("num_nodes", C.c_uint32), ("num_chain_nodes", C.c_uint32), ("num_records", C.c_uint32),
                ("depth", C.c_uint32), ("grid_dim", C.c_uint32 * 3), ("grid_origin", C.c_float * 3),
                ("grid_inv", C.c_float * 3), ("grid_off", C.c_float * 3)]


BOUNCE_CLASSES = 25      # records per leaf in rt_bounce_class_entries_host's table
BOUNCE_CLASS_FULL = 24   # ... of which this one is the leaf's full record


class BounceClassInfo(C.Structure):
    _fields_ = [("form", C.c_uint32), ("num_records", C.c_uint32), ("num_class_nodes", C.c_uint32),
                ("first_class_node", C.c_uint32)]


class GlibcRand(C.Structure):
    _fields_ = [("r", C.c_int32 * 34), ("idx", C.c_uint32)]


# numpy views of the RNG-state layout: 12 uint32 words per state (d, v0..v4, flags, extra, pad, double)
STATE_WORDS = 12
assert C.sizeof(CurandState) == 48
assert C.sizeof(InputStruct) == 72
assert C.sizeof(HittableDesc) == 40
assert C.sizeof(MaterialDesc) == 48
assert C.sizeof(TextureDesc) == 32


def make_inputs(origin, orientation, up, far_plane, near_plane, fov, bg_start, bg_end) -> InputStruct:
    s = InputStruct()
    s.origin[:] = [float(v) for v in origin]
    s.orientation[:] = [float(v) for v in orientation]
    s.up[:] = [float(v) for v in up]
    s.far_plane = far_plane
    s.near_plane = near_plane
    s.fov = fov
    s.background_start[:] = [float(v) for v in bg_start]
    s.background_end[:] = [float(v) for v in bg_end]
    return s


def states_as_words(states: np.ndarray) -> np.ndarray:
    """View an (N,) buffer of 48-byte states as (N, 12) uint32."""
    return states.view(np.uint32).reshape(-1, STATE_WORDS)
