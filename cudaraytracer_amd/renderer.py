"""Host-side mirror of the reference's render caller (CudaLayer, Cuda/CudaLayer.cpp) over the C ABI.

`Renderer` owns the device framebuffer and RNG-state buffers (InitCudaBuffers, CudaLayer.cpp:68-74), seeds
the RNG (RunCudaInit → RenderInit, CudaLayer.cpp:93-101), holds the device scene (GenerateWorld,
CudaLayer.cpp:103-256) and renders frames (RunCudaUpdate → LaunchKernel, CudaLayer.cpp:372-375).  Device
memory is allocated through torch (plumbing only); every compute step is a librt_hip.so call.
"""
from __future__ import annotations

import ctypes as C

import numpy as np
import torch

from . import abi
from ._lib import RTError, check, lib
from .scenes import Scene


class DeviceScene:
    """rt_scene handle (device-resident BVH + primitive + material tables)."""

    def __init__(self, scene: Scene | None = None, reference_graph: int | None = None):
        L = lib()
        self.handle = C.c_void_p()
        self.scene = scene
        if reference_graph is not None:
            check(L.rt_scene_from_reference_graph(C.c_void_p(reference_graph), C.byref(self.handle)),
                  "rt_scene_from_reference_graph")
        else:
            self._desc = scene.desc()
            check(L.rt_scene_create(C.byref(self._desc), C.byref(self.handle)), "rt_scene_create")

    def info(self) -> abi.SceneInfo:
        out = abi.SceneInfo()
        check(lib().rt_scene_get_info(self.handle, C.byref(out)), "rt_scene_get_info")
        return out

    def update_materials(self, materials) -> None:
        check(lib().rt_scene_update_materials(self.handle, C.cast(materials, C.POINTER(abi.MaterialDesc)),
                                              len(materials)), "rt_scene_update_materials")

    def edited(self, hittables) -> "DeviceScene":
        """A new device scene with this one's materials and images and the given hittable list (rt_scene_edit): the
        same count and order, so primitive ids keep their meaning; the uploaded texels are shared, not copied.  Both
        scenes stay valid and are closed independently."""
        from .scenes import _hittable_array
        new = DeviceScene.__new__(DeviceScene)
        new.handle = C.c_void_p()
        arr = _hittable_array(hittables)
        new.scene = None
        if self.scene is not None:
            copy = (abi.HittableDesc * len(arr)).from_buffer_copy(arr)
            new.scene = Scene(copy, self.scene.materials, self.scene.images)
        check(lib().rt_scene_edit(self.handle, arr, len(arr), C.byref(new.handle)), "rt_scene_edit")
        return new

    # rt_query_rays' outputs: name -> (trailing shape, dtype)
    QUERY_OUTPUTS = {"normal_depth": ((4,), torch.float32), "albedo": ((4,), torch.float32), "prim_id": ((), torch.int32),
                     "uv": ((2,), torch.float32), "material": ((), torch.int32), "hits": ((2,), torch.int32)}

    def query(self, rays, outputs=("normal_depth", "albedo", "prim_id", "uv", "material", "hits"),
              rays_per_lane: int = 0) -> dict:
        """Closest hit and hit record of rays of the caller's own (rt_query_rays), asynchronous on torch's current
        stream.  rays: (n, 2, 4) float32, (origin, -), (direction, -) per ray — a torch tensor on the device, or a numpy
        array (uploaded to the current device).  Returns {name: tensor} for the outputs asked for: normal_depth (n, 4),
        albedo (n, 4), prim_id (n,), uv (n, 2), material (n,), hits (n, 2) (include/rt_hip.h, rt_query_args)."""
        names = tuple(outputs)
        unknown = [o for o in names if o not in self.QUERY_OUTPUTS]
        if unknown or not names or len(set(names)) != len(names):
            raise ValueError(f"outputs must be distinct names out of {tuple(self.QUERY_OUTPUTS)}, not {names!r}")
        if isinstance(rays, np.ndarray):
            rays = torch.from_numpy(np.array(rays, dtype=np.float32, order="C")).cuda()  # (a copy: the caller's may be read-only)
        if rays.dtype != torch.float32 or rays.dim() != 3 or tuple(rays.shape[1:]) != (2, 4) or not rays.is_cuda:
            raise ValueError("rays must be a float32 (n, 2, 4) tensor on the device")
        rays = rays.contiguous()
        n = rays.shape[0]
        out = {o: torch.empty((n,) + self.QUERY_OUTPUTS[o][0], dtype=self.QUERY_OUTPUTS[o][1], device=rays.device)
               for o in names}
        if n == 0:
            return out
        a = abi.QueryArgs()
        a.rays = rays.data_ptr()
        for o in names:
            setattr(a, o, out[o].data_ptr())
        a.n, a.rays_per_lane = n, rays_per_lane
        stream = torch.cuda.current_stream(rays.device).cuda_stream
        check(lib().rt_query_rays(self.handle, C.byref(a), C.c_void_p(stream)), "rt_query_rays")
        return out

    def occluded(self, rays, blocker: bool = False, rays_per_lane: int = 0):
        """Is anything hit within each ray's own range (rt_occluded_rays)?  Asynchronous on torch's current stream.
        rays: (n, 2, 4) float32, (origin, tmin), (direction, tmax) per ray — a torch tensor on the device, or a numpy
        array (uploaded to the current device); t is in units of |direction|.  Returns a bool (n,) tensor, or with
        blocker=True the pair (occluded, blocker): int32 (n,), the index in the scene's hittables of a primitive that
        the ray hits within its range (not necessarily the nearest), -1 where nothing is hit."""
        if isinstance(rays, np.ndarray):
            rays = torch.from_numpy(np.array(rays, dtype=np.float32, order="C")).cuda()  # (a copy: the caller's may be read-only)
        if rays.dtype != torch.float32 or rays.dim() != 3 or tuple(rays.shape[1:]) != (2, 4) or not rays.is_cuda:
            raise ValueError("rays must be a float32 (n, 2, 4) tensor on the device")
        rays = rays.contiguous()
        n = rays.shape[0]
        occ = torch.empty((n,), dtype=torch.bool, device=rays.device)  # (one byte per element: the kernel writes 0 / 1)
        blk = torch.empty((n,), dtype=torch.int32, device=rays.device) if blocker else None
        if n:
            a = abi.OcclusionArgs()
            a.rays, a.occluded = rays.data_ptr(), occ.data_ptr()
            if blocker:
                a.blocker = blk.data_ptr()
            a.n, a.rays_per_lane = n, rays_per_lane
            stream = torch.cuda.current_stream(rays.device).cuda_stream
            check(lib().rt_occluded_rays(self.handle, C.byref(a), C.c_void_p(stream)), "rt_occluded_rays")
        return (occ, blk) if blocker else occ

    def radiance(self, rays, samples: int = 1, depth: int = 8, sample_base: int = 0, stream_ids=None, seed: int = 1984,
                 frame: int = 0, background=((1.0, 1.0, 1.0), (0.5, 0.7, 1.0)), mean: bool = True, rays_per_lane: int = 0,
                 left_to_right: bool = False, direct_light: bool = False):
        """Path-traced radiance along rays of the caller's own (rt_radiance_rays), asynchronous on torch's current
        stream.  rays: (n, 2, 4) float32, (origin, -), (direction, -) per ray — a torch tensor on the device, or a numpy
        array (uploaded to the current device).  Ray i takes `samples` paths of at most `depth` bounces on the Philox
        stream (seed, stream_ids[i] or i, frame), samples sample_base .. sample_base + samples - 1.  stream_ids: a
        uint32 / int32 (n,) device tensor (the values' 32 bits are the ids), e.g. camera_rays' pixel_index.
        background: (start, end) of the sky's blend.  Returns a float32 (n, 4) tensor: mean=True (r, g, b, 1), the
        average of the samples; mean=False (r, g, b, samples), their fixed-point sum, which adds into an accumulation
        buffer as a frame's samples do.  direct_light=True (RT_RADIANCE_DIRECT_LIGHT): every Lambertian vertex also
        connects to a point sampled on one of the scene's light rectangles (scenes.scene_lights) with a shadow ray —
        the same expectation with far less noise where the lights are small; depth is then at most 4096."""
        if isinstance(rays, np.ndarray):
            rays = torch.from_numpy(np.array(rays, dtype=np.float32, order="C")).cuda()  # (a copy: the caller's may be read-only)
        if rays.dtype != torch.float32 or rays.dim() != 3 or tuple(rays.shape[1:]) != (2, 4) or not rays.is_cuda:
            raise ValueError("rays must be a float32 (n, 2, 4) tensor on the device")
        rays = rays.contiguous()
        n = rays.shape[0]
        if stream_ids is not None:
            if (stream_ids.dtype not in (torch.int32, torch.uint32) or tuple(stream_ids.shape) != (n,)
                    or stream_ids.device != rays.device):
                raise ValueError("stream_ids must be a 32-bit integer (n,) tensor on the rays' device")
            stream_ids = stream_ids.contiguous()
        out = torch.empty((n, 4), dtype=torch.float32, device=rays.device)
        if n:
            a = abi.RadianceArgs()
            a.rays = rays.data_ptr()
            if mean:
                a.mean = out.data_ptr()
            else:
                a.sum = out.data_ptr()
            if stream_ids is not None:
                a.stream_ids = stream_ids.data_ptr()
            a.n, a.rays_per_lane, a.samples_per_ray, a.sample_base, a.max_depth = n, rays_per_lane, samples, sample_base, depth
            a.flags = (abi.RT_FLAG_RIUS_LEFT_TO_RIGHT if left_to_right else 0) | (abi.RT_RADIANCE_DIRECT_LIGHT if direct_light else 0)
            a.rng_seed, a.rng_frame = seed, frame
            a.background_start[:] = [float(v) for v in background[0]]
            a.background_end[:] = [float(v) for v in background[1]]
            stream = torch.cuda.current_stream(rays.device).cuda_stream
            check(lib().rt_radiance_rays(self.handle, C.byref(a), C.c_void_p(stream)), "rt_radiance_rays")
        return out

    def adaptive_samples(self, pixels, inputs: abi.InputStruct, width: int, height: int, depth: int = 8, samples=None,
                         count=None, history=None, moments=None, accum=None, samples_per_pixel: int = 1,
                         max_samples: int = 16, sample_base: int = 1, max_history: int = 32, seed: int = 1984,
                         frame: int = 0, rays_per_lane: int = 0, left_to_right: bool = False, counters=None,
                         direct_light: bool = False) -> None:
        """The extra samples of a pixel list, traced and merged in place (rt_adaptive_samples), asynchronous on torch's
        current stream.  pixels: a 32-bit integer (capacity,) device tensor of global pixel indices y * width + x, each
        at most once; samples: the same shape, paths per entry (else samples_per_pixel each, at most max_samples);
        count: a 32-bit integer device tensor whose first word is the number of entries (adaptive_select's; the host does
        not read it), else every element of `pixels` is one.  Path j of an entry is sample sample_base + j of that
        pixel's Philox stream (seed, pixel, frame).  Targets, float32 device tensors of the whole frame: history
        (H, W, 4) with or without moments (H, W, 2), blended as further 1-spp frames of rt_temporal_moments would be;
        accum (H, W, 4), added to as RT_FLAG_ACCUMULATE does.  direct_light=True (RT_RADIANCE_DIRECT_LIGHT): every
        path is the one radiance(..., direct_light=True) runs for that sample's camera ray with the pixel as its stream
        id."""
        if pixels.dtype not in (torch.int32, torch.uint32) or pixels.dim() != 1 or not pixels.is_cuda or not pixels.is_contiguous():
            raise ValueError("pixels must be a contiguous 32-bit integer (capacity,) tensor on the device")
        if samples is not None and (samples.dtype not in (torch.int32, torch.uint32) or samples.shape != pixels.shape
                                    or samples.device != pixels.device or not samples.is_contiguous()):
            raise ValueError("samples must be a contiguous 32-bit integer tensor of pixels' shape on its device")
        if count is not None and (count.dtype not in (torch.int32, torch.uint32) or count.numel() < 1
                                  or count.device != pixels.device):
            raise ValueError("count must be a 32-bit integer tensor on the pixels' device")
        for name, plane, last in (("history", history, 4), ("moments", moments, 2), ("accum", accum, 4)):
            if plane is not None and (plane.dtype != torch.float32 or plane.numel() != width * height * last
                                      or plane.device != pixels.device or not plane.is_contiguous()):
                raise ValueError(f"{name} must be a contiguous float32 tensor of {height} x {width} x {last} on the pixels' device")
        a = abi.AdaptiveSamplesArgs()
        a.pixels = pixels.data_ptr()
        for name, t in (("samples", samples), ("count", count), ("history", history), ("moments", moments),
                        ("accum", accum), ("counters", counters)):
            if t is not None:
                setattr(a, name, t.data_ptr())
        a.capacity, a.width, a.height = pixels.shape[0], width, height
        a.samples_per_pixel, a.max_samples, a.sample_base = samples_per_pixel, max_samples, sample_base
        a.max_depth, a.max_history, a.rays_per_lane = depth, max_history, rays_per_lane
        a.flags = (abi.RT_FLAG_RIUS_LEFT_TO_RIGHT if left_to_right else 0) | (abi.RT_RADIANCE_DIRECT_LIGHT if direct_light else 0)
        a.rng_seed, a.rng_frame = seed, frame
        a.inputs = inputs
        stream = torch.cuda.current_stream(pixels.device).cuda_stream
        check(lib().rt_adaptive_samples(self.handle, C.byref(a), C.c_void_p(stream)), "rt_adaptive_samples")

    def temporal_gradient(self, prev_color, inputs: abi.InputStruct, width: int, height: int, depth: int = 8,
                          stride: int = 3, offset=(0, 0), samples_per_pixel: int = 1, seed: int = 1984, frame: int = 0,
                          gradient=None, resample=None, pixel=None, rays_per_lane: int = 0,
                          left_to_right: bool = False, counters=None, direct_light: bool = False):
        """A past Philox frame's samples traced again in this scene and compared with what that frame stored
        (rt_temporal_gradient), asynchronous on torch's current stream.  prev_color: that frame's radiance plane, a
        float32 device tensor of H x W x 4; inputs, seed, frame, samples_per_pixel, depth and left_to_right are that
        frame's.  One pixel per stride x stride stratum, at `offset` = (offset_x, offset_y) inside it.  Outputs, device
        tensors over the ceil(H / stride) x ceil(W / stride) strata: gradient (.., 2) float32 (allocated when None),
        resample (.., 4) float32 and pixel (..) 32-bit integers, both optional.  direct_light=True
        (RT_RADIANCE_DIRECT_LIGHT): that frame was drawn with light sampling, and is traced again with it.  Returns
        gradient."""
        if (prev_color.dtype != torch.float32 or prev_color.numel() != width * height * 4 or not prev_color.is_cuda
                or not prev_color.is_contiguous()):
            raise ValueError(f"prev_color must be a contiguous float32 tensor of {height} x {width} x 4 on the device")
        if not 1 <= stride <= 8:
            raise ValueError("stride must be 1..8")
        sw, sh = -(-width // stride), -(-height // stride)
        if gradient is None:
            gradient = torch.empty((sh, sw, 2), dtype=torch.float32, device=prev_color.device)
        for name, t, dtypes, last in (("gradient", gradient, (torch.float32,), 2), ("resample", resample, (torch.float32,), 4),
                                      ("pixel", pixel, (torch.int32, torch.uint32), 1)):
            if t is not None and (t.dtype not in dtypes or t.numel() != sw * sh * last or t.device != prev_color.device
                                  or not t.is_contiguous()):
                raise ValueError(f"{name} must be a contiguous tensor of {sh} x {sw} x {last} on prev_color's device")
        a = abi.TemporalGradientArgs()
        a.prev_color, a.gradient = prev_color.data_ptr(), gradient.data_ptr()
        for name, t in (("resample", resample), ("pixel", pixel), ("counters", counters)):
            if t is not None:
                setattr(a, name, t.data_ptr())
        a.width, a.height, a.stride, a.offset_x, a.offset_y = width, height, stride, int(offset[0]), int(offset[1])
        a.samples_per_pixel, a.max_depth, a.rays_per_lane = samples_per_pixel, depth, rays_per_lane
        a.flags = (abi.RT_FLAG_RIUS_LEFT_TO_RIGHT if left_to_right else 0) | (abi.RT_RADIANCE_DIRECT_LIGHT if direct_light else 0)
        a.rng_seed, a.rng_frame = seed, frame
        a.tiling = abi.Tiling(max(height, 1), 1, 0, height)
        a.inputs = inputs
        stream = torch.cuda.current_stream(prev_color.device).cuda_stream
        check(lib().rt_temporal_gradient(self.handle, C.byref(a), C.c_void_p(stream)), "rt_temporal_gradient")
        return gradient

    def close(self) -> None:
        if self.handle:
            lib().rt_scene_destroy(self.handle)
            self.handle = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def set_tile_occlusion(on: bool) -> bool:
    """rt_set_tile_occlusion for the calling thread: whether the v3 kernels' tile entry records leave out candidates
    hidden behind a covering sphere (default on; same pixels either way).  Returns the previous setting."""
    prev = lib().rt_set_tile_occlusion(1 if on else 0)
    if prev < 0:
        check(prev, "rt_set_tile_occlusion")
    return bool(prev)


def set_bounce_classes(form: int) -> int:
    """rt_set_bounce_classes for the calling thread: the direction-class records of the v3 kernels' bounce entries that
    scenes created afterwards carry (0 = none, 1 = the existing chain nodes, 2 = re-paired; same pixels in every form).
    Returns the previous value."""
    prev = lib().rt_set_bounce_classes(int(form))
    if prev < 0:
        check(prev, "rt_set_bounce_classes")
    return prev


def camera_rays(inputs: abi.InputStruct, width: int, height: int, pixels=None, jitter=(0.5, 0.5), sample: int = 0,
                seed: int = 1984, frame: int = 0, tiling: abi.Tiling | None = None, device=None):
    """The library's own camera rays as a ray batch (rt_camera_rays), asynchronous on torch's current stream: the rays
    the render kernels trace, bit for bit.  pixels=None: one ray per pixel of the frame, row-major (of this rank's
    rows with a `tiling`); pixels: a 32-bit integer (n,) device tensor (or a sequence, uploaded) of global pixel
    indices y * width + x, one ray each.  jitter: a pair (xi1, xi2) in pixel units — (0.5, 0.5) is the pixel centre,
    rt_gbuffer's ray — or "philox": the jitter rt_render draws for that pixel's sample `sample` with
    RT_FLAG_RNG_PHILOX, seed and frame.  Returns (rays, pixel_index): float32 (n, 2, 4) as (origin, 0.001),
    (direction, FLT_MAX) — valid for DeviceScene.query, .occluded and .radiance as it is — and int32 (n,), each ray's
    global pixel index (DeviceScene.radiance's stream_ids)."""
    if pixels is not None and not isinstance(pixels, torch.Tensor):
        pixels = torch.from_numpy(np.array(pixels, dtype=np.int64).astype(np.uint32).view(np.int32)).cuda()
    if pixels is not None:
        if pixels.dtype not in (torch.int32, torch.uint32) or pixels.dim() != 1 or not pixels.is_cuda:
            raise ValueError("pixels must be a 32-bit integer (n,) tensor on the device")
        pixels = pixels.contiguous()
        device = pixels.device
    elif device is None:
        device = torch.device("cuda", torch.cuda.current_device())
    t = tiling if tiling is not None else abi.Tiling(max(height, 1), 1, 0, height)
    n = pixels.shape[0] if pixels is not None else t.local_rows * width
    rays = torch.empty((n, 2, 4), dtype=torch.float32, device=device)
    index = torch.empty((n,), dtype=torch.int32, device=device)
    if n:
        a = abi.CameraRaysArgs()
        a.rays, a.pixel_index = rays.data_ptr(), index.data_ptr()
        if pixels is not None:
            a.pixels = pixels.data_ptr()
        a.n, a.width, a.height, a.tiling, a.inputs = n, width, height, t, inputs
        if isinstance(jitter, str):
            if jitter != "philox":
                raise ValueError('jitter must be a pair (xi1, xi2) or "philox"')
            a.flags, a.sample, a.rng_seed, a.rng_frame = abi.RT_CAMERA_JITTER_PHILOX, sample, seed, frame
        else:
            a.xi1, a.xi2 = float(jitter[0]), float(jitter[1])
        stream = torch.cuda.current_stream(device).cuda_stream
        check(lib().rt_camera_rays(C.byref(a), C.c_void_p(stream)), "rt_camera_rays")
    return rays, index


def band_rows_of(height: int, band_rows: int, num_ranks: int, rank: int) -> list[int]:
    """Global rows owned by `rank` under block-cyclic row bands (rt_tiling, include/rt_hip.h)."""
    rows = []
    b = rank
    while b * band_rows < height:
        rows.extend(range(b * band_rows, min(height, (b + 1) * band_rows)))
        b += num_ranks
    return rows


class Renderer:
    """One rank's share of a W×H image (all of it when num_ranks = 1)."""

    def __init__(self, width: int, height: int, device: int | str = 0, band_rows: int | None = None,
                 num_ranks: int = 1, rank: int = 0, rng: str = "xorwow", state_layout: str = "curand"):
        """rng = "xorwow": the reference's per-pixel cuRAND XORWOW state (parity mode); "philox": stateless
        per-pixel Philox4x32-10 streams (RT_FLAG_RNG_PHILOX, perf mode, no RNG bytes in HBM).
        state_layout (XORWOW): "curand" = the reference's 48-byte curandState per pixel; "soa" = the same
        states as six uint32 planes (RT_FLAG_STATE_SOA, 24 bytes per pixel)."""
        if rng not in ("xorwow", "philox"):
            raise ValueError(f"rng must be 'xorwow' or 'philox', not {rng!r}")
        if state_layout not in ("curand", "soa"):
            raise ValueError(f"state_layout must be 'curand' or 'soa', not {state_layout!r}")
        self.state_layout = state_layout
        self.rng = rng
        self.seed = 1984  # Kernel.cu:175 seed base; the Philox key in perf mode
        self.frame = 0    # Philox frame counter (the XORWOW streams carry over in `state` instead)
        if not torch.cuda.is_available():
            raise RTError("no HIP device visible: librt_hip.so renders on MI355X only")
        self.device = torch.device("cuda", device) if isinstance(device, int) else torch.device(device)
        torch.cuda.set_device(self.device)
        check(lib().rt_set_device(self.device.index or 0), "rt_set_device")
        self.width, self.height = width, height
        self.band_rows = band_rows or height
        self.num_ranks, self.rank = num_ranks, rank
        self.rows = band_rows_of(height, self.band_rows, num_ranks, rank)
        self.local_rows = len(self.rows)
        n = width * self.local_rows
        # InitCudaBuffers (CudaLayer.cpp:68-74): RGBA8 framebuffer + one 48-byte curandState per pixel
        # (none in Philox mode)
        self.pos = torch.zeros(n, dtype=torch.int32, device=self.device)
        words = n * abi.STATE_WORDS if state_layout == "curand" else 6 * int(lib().rt_soa_plane_words(width, self.local_rows))
        self.state = torch.zeros(words, dtype=torch.int32, device=self.device) if rng == "xorwow" else None
        self.counters = torch.zeros(abi.COUNTERS_WORDS, dtype=torch.int64, device=self.device)
        self.radiance = None
        self.accum = None
        self._accum_restart = False  # the next accumulating frame restarts the sums (RT_FLAG_ACCUMULATE_RESET)
        self.normal_depth = self.albedo = self.prim_id = None  # gbuffer(): allocated on first use
        self.denoised = None          # denoise(): the float result (local_rows × W × 4)
        self._denoise_scratch = None  # ... its ping-pong planes, allocated once
        self._denoise_pos = None
        # gbuffer(keep_previous=True): the frame before's planes and camera; temporal(): the accumulated colour
        self.prev_normal_depth = self.prev_prim_id = self.prev_inputs = None
        self._gbuffer_inputs = None
        self.history = None          # temporal(): (local_rows × W × 4) float32, rgb + history length
        self._history_spare = None   # ... the plane the next call writes (the two ping-pong)
        self.motion = None           # temporal(motion=True): (local_rows × W × 2) float32
        self._temporal_pos = None
        self._prim_motion = None     # temporal(prim_motion=...): the device table of the last call
        self.moments = None          # temporal(moments=True): (local_rows × W × 2) float32, luminance moments (m1, m2)
        self._moments_spare = None   # ... the plane the next call writes
        self.denoised_variance = None          # denoise_variance(): (local_rows × W × 4) float32, rgb + variance
        self._denoise_variance_scratch = None  # ... its planes, allocated once
        self._denoise_variance_pos = None
        # adaptive_select(): the pixel list, its sample counts and (listed pixels, samples) on the device
        self.adaptive_pixels = self.adaptive_samples = self.adaptive_count = None
        self._adaptive_scratch = None
        # temporal_gradient(): the (strata rows × strata columns × 2) plane of the last call, the frame that wrote the
        # `radiance` plane (inputs, seed, frame, spp, flags; None after an XORWOW frame) and the calls so far
        self.gradient = None
        self._radiance_frame = None
        self._gradient_calls = 0
        # render_direct(): every pixel in ascending order, the frame's sums and the divisor, allocated on first use
        self._all_pixels = self._direct_accum = self._direct_spp = None

    def tiling(self) -> abi.Tiling:
        return abi.Tiling(self.band_rows, self.num_ranks, self.rank, self.local_rows)

    def stream(self) -> int:
        return torch.cuda.current_stream(self.device).cuda_stream

    def render_init(self, seed_base: int = 1984) -> None:
        """RenderInit: curand_init(seed_base + global pixel index, 0, 0) (Kernel.cu:166-176); in Philox mode
        the seed becomes the Philox key and the frame counter restarts."""
        self.seed, self.frame = seed_base, 0
        if self.state is None:
            return
        t = self.tiling()
        init = lib().rt_render_init_soa if self.state_layout == "soa" else lib().rt_render_init
        check(init(C.c_void_p(self.state.data_ptr()), self.width, self.height, C.byref(t), seed_base,
                   C.c_void_p(self.stream())), "rt_render_init")

    def render(self, scene: DeviceScene, spp: int, max_depth: int, inputs: abi.InputStruct, flags: int = 0,
               radiance: bool = False, count: bool = True, frame: int | None = None) -> torch.Tensor:
        """One frame (Kernel.cu:102-158), asynchronous on torch's current stream; returns `pos`.  Philox
        mode draws frame `frame` (default: the next frame counter value) of every pixel's stream."""
        if radiance and self.radiance is None:
            self.radiance = torch.zeros(self.width * self.local_rows * 4, dtype=torch.float32, device=self.device)
        if flags & abi.RT_FLAG_ACCUMULATE:
            if self.accum is None:
                # zeroed once: the first frame (RT_FLAG_ACCUMULATE_RESET) writes every pixel it renders, but with
                # RT_FLAG_FAITHFUL_GRID the pixels outside whole 16×16 blocks are never rendered and must read 0
                self.accum = torch.zeros(self.width * self.local_rows * 4, dtype=torch.float32, device=self.device)
                self._accum_restart = True
            if self._accum_restart:
                flags |= abi.RT_FLAG_ACCUMULATE_RESET
                self._accum_restart = False
        a = abi.RenderArgs()
        a.pos = self.pos.data_ptr()
        a.radiance = self.radiance.data_ptr() if radiance else None
        a.accum = self.accum.data_ptr() if self.accum is not None and flags & abi.RT_FLAG_ACCUMULATE else None
        a.state = self.state.data_ptr() if self.state is not None else None
        a.counters = self.counters.data_ptr() if count else None
        a.width, a.height = self.width, self.height
        a.samples_per_pixel, a.max_depth = spp, max_depth
        if self.rng == "philox":
            flags |= abi.RT_FLAG_RNG_PHILOX
            if frame is None:
                frame = self.frame
                if not flags & abi.RT_FLAG_NO_STATE_WRITEBACK:
                    self.frame += 1  # the next frame draws fresh numbers, as the XORWOW streams advance
            a.rng_seed, a.rng_frame = self.seed, frame
        if self.state_layout == "soa" and self.state is not None:
            flags |= abi.RT_FLAG_STATE_SOA
        a.flags = flags
        a.tiling = self.tiling()
        a.inputs = inputs
        check(lib().rt_render(scene.handle, C.byref(a), C.c_void_p(self.stream())), "rt_render")
        if radiance:  # what temporal_gradient() needs to trace this frame's paths again
            self._radiance_frame = ((abi.InputStruct.from_buffer_copy(inputs), self.seed, frame, spp, flags)
                                    if self.rng == "philox" else None)
        return self.pos

    def render_direct(self, scene: DeviceScene, inputs: abi.InputStruct, spp: int = 1, depth: int = 8,
                      direct_light: bool = True, left_to_right: bool = False) -> torch.Tensor:
        """One whole Philox frame through the fused pass (rt_adaptive_samples over every pixel, samples 0 .. spp - 1,
        spp in 1..16, into a zeroed sum plane), with light sampling (RT_RADIANCE_DIRECT_LIGHT) unless direct_light is
        False; asynchronous on torch's current stream.  Stores `radiance` = (the samples' sum / spp, 1) per pixel — the
        plane temporal() and temporal_gradient() read — and records the frame, its flag bits included, so that
        temporal_gradient() traces it again with the same estimator and adaptive() continues it.  Draws the next frame
        counter value, as render() does.  Whole frames of a Philox renderer only; nothing is synchronised.  Returns
        `radiance`."""
        if self.rng != "philox":
            raise RTError("render_direct: the renderer's rng must be 'philox'")
        if self.num_ranks != 1:
            raise RTError("render_direct: whole frames only (num_ranks = 1)")
        if not 1 <= spp <= 16:
            raise ValueError("spp must be 1..16")
        n = self.width * self.height
        if self._all_pixels is None:
            self._all_pixels = torch.arange(n, dtype=torch.int32, device=self.device)
            self._direct_accum = torch.zeros((n, 4), dtype=torch.float32, device=self.device)
            self._direct_spp = torch.zeros(1, dtype=torch.float32, device=self.device)
        if self.radiance is None:
            self.radiance = torch.zeros(n * 4, dtype=torch.float32, device=self.device)
        frame = self.frame
        self.frame += 1
        self._direct_accum.zero_()
        scene.adaptive_samples(self._all_pixels, inputs, self.width, self.height, depth, accum=self._direct_accum,
                               samples_per_pixel=spp, max_samples=16, sample_base=0, seed=self.seed, frame=frame,
                               left_to_right=left_to_right, direct_light=direct_light)
        out = self.radiance.view(n, 4)
        self._direct_spp.fill_(float(spp))
        # (a tensor divisor: a Python scalar would be turned into a multiplication by its reciprocal)
        torch.div(self._direct_accum[:, :3], self._direct_spp, out=out[:, :3])
        out[:, 3] = 1.0
        flags = (abi.RT_FLAG_RNG_PHILOX | (abi.RT_FLAG_RIUS_LEFT_TO_RIGHT if left_to_right else 0)
                 | (abi.RT_RADIANCE_DIRECT_LIGHT if direct_light else 0))
        self._radiance_frame = (abi.InputStruct.from_buffer_copy(inputs), self.seed, frame, spp, flags)
        return self.radiance

    def reset_accumulation(self) -> None:
        """Restart the progressive sums (camera move, scene edit): the next accumulating frame passes
        RT_FLAG_ACCUMULATE_RESET, which writes the accumulator without reading it — no fill kernel."""
        self._accum_restart = True

    def gbuffer(self, scene: DeviceScene, inputs: abi.InputStruct, keep_previous: bool = False):
        """First-hit G-buffer of this rank's rows (rt_gbuffer), asynchronous on torch's current stream: returns
        (normal_depth (rows, W, 4) float32, albedo (rows, W, 4) float32, prim_id (rows, W) int32), cached on the
        renderer.  No RNG draw: the states are untouched.  keep_previous: write into the renderer's second plane set,
        so the planes and camera of the call before stay available as prev_normal_depth, prev_prim_id and prev_inputs
        (what temporal() reprojects into); the default overwrites the one set in place."""
        if keep_previous and self.normal_depth is not None:
            spare_nd = self.prev_normal_depth if self.prev_normal_depth is not None else torch.zeros_like(self.normal_depth)
            spare_id = self.prev_prim_id if self.prev_prim_id is not None else torch.zeros_like(self.prim_id)
            self.prev_normal_depth, self.normal_depth = self.normal_depth, spare_nd
            self.prev_prim_id, self.prim_id = self.prim_id, spare_id
            self.prev_inputs = self._gbuffer_inputs
        self._gbuffer_inputs = abi.InputStruct.from_buffer_copy(inputs)
        if self.normal_depth is None:
            shape = (self.local_rows, self.width)
            self.normal_depth = torch.zeros(shape + (4,), dtype=torch.float32, device=self.device)
            self.albedo = torch.zeros(shape + (4,), dtype=torch.float32, device=self.device)
            self.prim_id = torch.zeros(shape, dtype=torch.int32, device=self.device)
        a = abi.GBufferArgs()
        a.normal_depth, a.albedo, a.prim_id = self.normal_depth.data_ptr(), self.albedo.data_ptr(), self.prim_id.data_ptr()
        a.width, a.height = self.width, self.height
        a.tiling = self.tiling()
        a.inputs = inputs
        check(lib().rt_gbuffer(scene.handle, C.byref(a), C.c_void_p(self.stream())), "rt_gbuffer")
        return self.normal_depth, self.albedo, self.prim_id

    def denoise(self, iterations: int = 3, sigma_c: float = 0.6, sigma_n: float = 0.1, sigma_z: float = 0.05,
                demodulate: bool = True, source: str = "radiance") -> np.ndarray:
        """Edge-avoiding à-trous filter (rt_denoise) of the last frame's `radiance` (render(..., radiance=True)) or
        `accum` (RT_FLAG_ACCUMULATE) plane, or of temporal()'s `history` (source="history"), guided by the last
        gbuffer(); whole frames only (num_ranks = 1).  Returns
        the RGBA8 image like image() and keeps the float result in `self.denoised`."""
        pos = self.denoise_async(iterations, sigma_c, sigma_n, sigma_z, demodulate, source)
        return pos.cpu().numpy().view(np.uint32).reshape(self.local_rows, self.width)

    def denoise_async(self, iterations: int = 3, sigma_c: float = 0.6, sigma_n: float = 0.1, sigma_z: float = 0.05,
                      demodulate: bool = True, source: str = "radiance") -> torch.Tensor:
        """denoise() without the copy to the host: asynchronous on torch's current stream; returns the device RGBA8
        framebuffer (as render() returns `pos`)."""
        if source not in ("radiance", "accum", "history"):
            raise ValueError(f"source must be 'radiance', 'accum' or 'history', not {source!r}")
        color = {"radiance": self.radiance, "accum": self.accum, "history": self.history}[source]
        if color is None:
            raise RTError(f"denoise: no {source} plane (render with radiance=True / RT_FLAG_ACCUMULATE, or call "
                          "temporal(), first)")
        if self.normal_depth is None:
            raise RTError("denoise: no G-buffer (call gbuffer() first)")
        L = lib()
        n = self.width * self.local_rows
        if self.denoised is None:
            self.denoised = torch.zeros((self.local_rows, self.width, 4), dtype=torch.float32, device=self.device)
            self._denoise_pos = torch.zeros(n, dtype=torch.int32, device=self.device)
        need = int(L.rt_denoise_scratch_bytes(self.width, self.height, 6))  # once, for any iteration count
        if self._denoise_scratch is None and need:
            self._denoise_scratch = torch.zeros(need, dtype=torch.uint8, device=self.device)
        a = abi.DenoiseArgs()
        a.color = color.data_ptr()
        a.normal_depth, a.albedo, a.prim_id = self.normal_depth.data_ptr(), self.albedo.data_ptr(), self.prim_id.data_ptr()
        a.out_color, a.pos = self.denoised.data_ptr(), self._denoise_pos.data_ptr()
        a.scratch = self._denoise_scratch.data_ptr() if self._denoise_scratch is not None else None
        a.width, a.height, a.iterations = self.width, self.height, iterations
        a.flags = (abi.RT_DENOISE_DEMODULATE if demodulate else 0) | (abi.RT_DENOISE_COLOR_IS_SUM if source == "accum" else 0)
        a.sigma_c, a.sigma_n, a.sigma_z = sigma_c, sigma_n, sigma_z
        a.tiling = self.tiling()
        check(L.rt_denoise(C.byref(a), C.c_void_p(self.stream())), "rt_denoise")
        return self._denoise_pos

    def temporal(self, max_history: int = 32, depth_tol: float = 0.05, normal_tol: float = 0.2,
                 source: str = "radiance", reset: bool = False, motion: bool = False, prim_motion=None,
                 moments: bool = False) -> torch.Tensor:
        """Reprojected temporal accumulation (rt_temporal) of the last frame's `radiance` or `accum` plane into
        `self.history` (rows, W, 4: rgb, history length), asynchronous on torch's current stream; whole frames only.
        Call once per frame after render() and gbuffer(..., keep_previous=True): the last call's history is looked up
        where this frame's surfaces were under prev_inputs.  The first call, or one without a previous G-buffer, behaves
        as reset=True.  motion=True also fills `self.motion` (rows, W, 2).  Returns the device RGBA8 buffer of the
        accumulated colour; denoise(source="history") filters it.
        prim_motion: the (n, 4) float32 per-hittable motion table of an object edit between the two frames
        (scenes.scene_motion; a torch tensor on this device or a numpy array, which is uploaded): the pass then runs as
        rt_temporal_dynamic and history follows the moved hittables.  None keeps the rt_temporal call.
        moments=True runs the pass as rt_temporal_moments (with or without the table): `self.moments` (rows, W, 2), the
        accumulated first and second moment of the luminance, ping-pongs beside the history; denoise_variance() reads
        it.  A call that finds no moments plane of the call before behaves as reset=True."""
        if source not in ("radiance", "accum"):
            raise ValueError(f"source must be 'radiance' or 'accum', not {source!r}")
        color = self.radiance if source == "radiance" else self.accum
        if color is None:
            raise RTError(f"temporal: no {source} plane (render with radiance=True / RT_FLAG_ACCUMULATE first)")
        if self.normal_depth is None or self._gbuffer_inputs is None:
            raise RTError("temporal: no G-buffer (call gbuffer() first)")
        shape = (self.local_rows, self.width)
        out = self._history_spare
        if out is None:
            out = torch.zeros(shape + (4,), dtype=torch.float32, device=self.device)
        if self._temporal_pos is None:
            self._temporal_pos = torch.zeros(self.width * self.local_rows, dtype=torch.int32, device=self.device)
        if motion and self.motion is None:
            self.motion = torch.zeros(shape + (2,), dtype=torch.float32, device=self.device)
        reset = reset or self.history is None or self.prev_normal_depth is None or self.prev_inputs is None
        reset = reset or (moments and self.moments is None)
        a = abi.TemporalArgs()
        a.color = color.data_ptr()
        a.normal_depth, a.prim_id = self.normal_depth.data_ptr(), self.prim_id.data_ptr()
        if not reset:
            a.prev_history = self.history.data_ptr()
            a.prev_normal_depth, a.prev_prim_id = self.prev_normal_depth.data_ptr(), self.prev_prim_id.data_ptr()
            a.prev_inputs = self.prev_inputs
        a.history = out.data_ptr()
        a.motion = self.motion.data_ptr() if motion else None
        a.pos = self._temporal_pos.data_ptr()
        a.width, a.height, a.max_history = self.width, self.height, max_history
        a.flags = (abi.RT_TEMPORAL_COLOR_IS_SUM if source == "accum" else 0) | (abi.RT_TEMPORAL_RESET if reset else 0)
        a.depth_tol, a.normal_tol = depth_tol, normal_tol
        a.tiling = self.tiling()
        a.inputs = self._gbuffer_inputs
        table = None
        if prim_motion is not None:
            table = prim_motion
            if not isinstance(table, torch.Tensor):
                table = torch.from_numpy(np.array(table, dtype=np.float32))
            if table.device != self.device or table.dtype != torch.float32 or not table.is_contiguous():
                table = table.to(device=self.device, dtype=torch.float32).contiguous()
            if table.numel() % 4:
                raise ValueError("temporal: prim_motion holds four floats per hittable")
            self._prim_motion = table  # (kept until the next call: the launch is asynchronous)
        table_ptr = C.c_void_p(table.data_ptr() if table is not None and table.numel() else None)
        if moments:
            out_m = self._moments_spare
            if out_m is None:
                out_m = torch.zeros(shape + (2,), dtype=torch.float32, device=self.device)
            if table is not None and not table.numel():
                raise ValueError("temporal: moments=True takes prim_motion=None or a table with entries")
            check(lib().rt_temporal_moments(C.byref(a), table_ptr, table.numel() // 4 if table is not None else 0,
                                            C.c_void_p(None if reset else self.moments.data_ptr()),
                                            C.c_void_p(out_m.data_ptr()), C.c_void_p(self.stream())), "rt_temporal_moments")
            self.moments, self._moments_spare = out_m, self.moments
        else:
            if table is None:
                check(lib().rt_temporal(C.byref(a), C.c_void_p(self.stream())), "rt_temporal")
            else:
                check(lib().rt_temporal_dynamic(C.byref(a), table_ptr, table.numel() // 4, C.c_void_p(self.stream())),
                      "rt_temporal_dynamic")
            if self.moments is not None:  # a frame without moments: the plane no longer belongs to the history
                self._moments_spare, self.moments = self.moments, None
        self.history, self._history_spare = out, self.history
        return self._temporal_pos

    def adaptive_select(self, tau: float = 0.1, min_history: int = 4, max_samples: int = 4, capacity: int | None = None,
                        lum_floor: float = 0.01, pixels_per_lane: int = 0):
        """Which pixels need how many more samples (rt_adaptive_select) by temporal(moments=True)'s `history` and
        `moments` and the last gbuffer()'s prim_id (misses are never listed), asynchronous on torch's current stream;
        whole frames only.  Returns the device tensors (pixels (capacity,) int32, samples (capacity,) int32, count (2,)
        int32): the first min(count[0], capacity) entries are the pixels y * width + x with k > 0 in ascending order and
        their k <= max_samples; count = (listed pixels in the frame, their k summed).  capacity defaults to the frame.
        The tensors are the renderer's (`adaptive_pixels`, `adaptive_samples`, `adaptive_count`) and are reused by the
        next call of the same capacity."""
        if self.history is None or self.moments is None:
            raise RTError("adaptive_select: no history and moments planes (call temporal(moments=True) first)")
        n = self.width * self.local_rows
        capacity = n if capacity is None else int(capacity)
        if self.adaptive_pixels is None or self.adaptive_pixels.shape[0] != capacity:
            self.adaptive_pixels = torch.zeros(capacity, dtype=torch.int32, device=self.device)
            self.adaptive_samples = torch.zeros(capacity, dtype=torch.int32, device=self.device)
        if self.adaptive_count is None:
            self.adaptive_count = torch.zeros(2, dtype=torch.int32, device=self.device)
            need = int(lib().rt_adaptive_select_scratch_bytes(self.width, self.height))
            self._adaptive_scratch = torch.zeros(max(need, 4), dtype=torch.uint8, device=self.device)
        a = abi.AdaptiveSelectArgs()
        a.history, a.moments = self.history.data_ptr(), self.moments.data_ptr()
        a.prim_id = self.prim_id.data_ptr() if self.prim_id is not None else None
        if capacity:
            a.pixels, a.samples = self.adaptive_pixels.data_ptr(), self.adaptive_samples.data_ptr()
        a.count, a.scratch = self.adaptive_count.data_ptr(), self._adaptive_scratch.data_ptr()
        a.width, a.height, a.capacity = self.width, self.height, capacity
        a.max_samples, a.min_history, a.tau, a.lum_floor = max_samples, min_history, tau, lum_floor
        a.pixels_per_lane = pixels_per_lane
        a.tiling = self.tiling()
        check(lib().rt_adaptive_select(C.byref(a), C.c_void_p(self.stream())), "rt_adaptive_select")
        return self.adaptive_pixels, self.adaptive_samples, self.adaptive_count

    def adaptive(self, scene: DeviceScene, inputs: abi.InputStruct, depth: int, tau: float = 0.1, min_history: int = 4,
                 max_samples: int = 4, capacity: int | None = None, frame: int | None = None, seed: int | None = None,
                 sample_base: int = 1, max_history: int = 32, lum_floor: float = 0.01,
                 direct_light: bool | None = None) -> torch.Tensor:
        """Adaptive sampling on the device: adaptive_select(), then DeviceScene.adaptive_samples() on the list, merged
        into the current `history` and `moments` planes in place.  Call after temporal(moments=True) and before
        denoise_variance(); whole frames only.  The extra samples of a pixel are samples sample_base .. of the Philox
        stream (seed, pixel, frame): with the defaults — the renderer's seed, the frame render() drew last, sample 1 on
        — they continue a 1-spp Philox frame.  max_history is temporal()'s.  Nothing is synchronised: returns the
        device `count` tensor (listed pixels, extra samples).  direct_light: trace the extra samples with light sampling
        (RT_RADIANCE_DIRECT_LIGHT); None takes what the recorded frame — the last render(radiance=True) or
        render_direct() — was drawn with."""
        if direct_light is None:
            direct_light = bool(self._radiance_frame is not None and self._radiance_frame[4] & abi.RT_RADIANCE_DIRECT_LIGHT)
        pixels, samples, count = self.adaptive_select(tau, min_history, max_samples, capacity, lum_floor)
        if pixels.shape[0]:
            scene.adaptive_samples(pixels, inputs, self.width, self.height, depth, samples=samples, count=count,
                                   history=self.history, moments=self.moments, max_samples=max_samples,
                                   sample_base=sample_base, max_history=max_history,
                                   seed=self.seed if seed is None else seed,
                                   frame=max(self.frame - 1, 0) if frame is None else frame,
                                   direct_light=direct_light)
        return count

    def temporal_gradient(self, scene: DeviceScene, depth: int, stride: int = 3, radius: int = 1, power: int = 4,
                          gain: float = 1.0, lum_floor: float = 0.01) -> torch.Tensor:
        """Cut stale history after a scene edit (rt_temporal_gradient, then rt_history_adapt): call after the edit and
        before the next render(), on frames with an edit only; whole frames only.  `scene` is the edited scene.  The
        last render(..., radiance=True) or render_direct() — its `radiance` plane, inputs, seed, frame number, spp, fill
        order and light sampling; it must
        have been a Philox frame, and `depth` must be the depth it was drawn with — is traced again in `scene` at one
        pixel per stride x stride stratum, and the current `history` plane's lengths are scaled in place by
        (1 - lambda)^power, lambda from the strata within `radius` of the pixel's.  The pixel's place in its stratum
        rotates through the stride^2 positions from call to call.  Nothing is synchronised: returns the device gradient
        plane (strata rows, strata columns, 2), also kept as `self.gradient`."""
        if self.radiance is None:
            raise RTError("temporal_gradient: no radiance plane (render with radiance=True first)")
        if self.history is None:
            raise RTError("temporal_gradient: no history plane (call temporal() first)")
        if self._radiance_frame is None:
            raise RTError("temporal_gradient: the last render was not a Philox frame (an XORWOW frame cannot be traced again)")
        if not 1 <= stride <= 8:
            raise ValueError("stride must be 1..8")
        inputs, seed, frame, spp, flags = self._radiance_frame
        sw, sh = -(-self.width // stride), -(-self.local_rows // stride)
        if self.gradient is None or tuple(self.gradient.shape) != (sh, sw, 2):
            self.gradient = torch.zeros((sh, sw, 2), dtype=torch.float32, device=self.device)
        turn = self._gradient_calls % (stride * stride)
        self._gradient_calls += 1
        a = abi.TemporalGradientArgs()
        a.prev_color, a.gradient = self.radiance.data_ptr(), self.gradient.data_ptr()
        a.width, a.height, a.stride, a.offset_x, a.offset_y = self.width, self.height, stride, turn % stride, turn // stride
        a.samples_per_pixel, a.max_depth = spp, depth
        a.flags = flags & (abi.RT_FLAG_RIUS_LEFT_TO_RIGHT | abi.RT_RADIANCE_DIRECT_LIGHT)
        a.rng_seed, a.rng_frame = seed, frame
        a.tiling = self.tiling()
        a.inputs = inputs
        check(lib().rt_temporal_gradient(scene.handle, C.byref(a), C.c_void_p(self.stream())), "rt_temporal_gradient")
        b = abi.HistoryAdaptArgs()
        b.gradient, b.history = self.gradient.data_ptr(), self.history.data_ptr()
        b.width, b.height, b.stride, b.radius, b.power = self.width, self.height, stride, radius, power
        b.gain, b.lum_floor = gain, lum_floor
        b.tiling = self.tiling()
        check(lib().rt_history_adapt(C.byref(b), C.c_void_p(self.stream())), "rt_history_adapt")
        return self.gradient

    def denoise_variance(self, iterations: int = 3, sigma_l: float = 1.0, sigma_n: float = 0.1, sigma_z: float = 0.05,
                         min_history: int = 4) -> np.ndarray:
        """Variance-guided à-trous filter (rt_denoise_variance) of temporal(moments=True)'s `history` and `moments`,
        guided by the last gbuffer(); whole frames only.  Returns the RGBA8 image like image() and keeps the float result
        (rgb, filtered variance) in `self.denoised_variance`."""
        pos = self.denoise_variance_async(iterations, sigma_l, sigma_n, sigma_z, min_history)
        return pos.cpu().numpy().view(np.uint32).reshape(self.local_rows, self.width)

    def denoise_variance_async(self, iterations: int = 3, sigma_l: float = 1.0, sigma_n: float = 0.1,
                               sigma_z: float = 0.05, min_history: int = 4) -> torch.Tensor:
        """denoise_variance() without the copy to the host: asynchronous on torch's current stream; returns the device
        RGBA8 framebuffer."""
        if self.history is None or self.moments is None:
            raise RTError("denoise_variance: no history and moments planes (call temporal(moments=True) first)")
        if self.normal_depth is None:
            raise RTError("denoise_variance: no G-buffer (call gbuffer() first)")
        L = lib()
        n = self.width * self.local_rows
        if self.denoised_variance is None:
            self.denoised_variance = torch.zeros((self.local_rows, self.width, 4), dtype=torch.float32, device=self.device)
            self._denoise_variance_pos = torch.zeros(n, dtype=torch.int32, device=self.device)
        need = int(L.rt_denoise_variance_scratch_bytes(self.width, self.height, 6))  # once, for any iteration count
        if self._denoise_variance_scratch is None and need:
            self._denoise_variance_scratch = torch.zeros(need, dtype=torch.uint8, device=self.device)
        a = abi.DenoiseVarianceArgs()
        a.color, a.moments = self.history.data_ptr(), self.moments.data_ptr()
        a.normal_depth, a.prim_id = self.normal_depth.data_ptr(), self.prim_id.data_ptr()
        a.out_color, a.pos = self.denoised_variance.data_ptr(), self._denoise_variance_pos.data_ptr()
        a.scratch = self._denoise_variance_scratch.data_ptr() if self._denoise_variance_scratch is not None else None
        a.width, a.height, a.iterations, a.min_history = self.width, self.height, iterations, min_history
        a.sigma_l, a.sigma_n, a.sigma_z = sigma_l, sigma_n, sigma_z
        a.tiling = self.tiling()
        check(L.rt_denoise_variance(C.byref(a), C.c_void_p(self.stream())), "rt_denoise_variance")
        return self._denoise_variance_pos

    def image(self) -> np.ndarray:
        """Local framebuffer as (local_rows, W) uint32 RGBA8 (row 0 = bottom of the image)."""
        return self.pos.cpu().numpy().view(np.uint32).reshape(self.local_rows, self.width)

    def states(self) -> np.ndarray:
        """The XORWOW states as (pixels, 12) rt_curand_state words (the SoA planes transposed into words 0-5;
        words 6-11, the Box-Muller fields the path never uses, zero)."""
        w = self.state.cpu().numpy().view(np.uint32)
        if self.state_layout == "curand":
            return w.reshape(-1, abi.STATE_WORDS)
        ly, x = np.divmod(np.arange(self.width * self.local_rows), self.width)
        idx = ((ly >> 3) * ((self.width + 7) >> 3) + (x >> 3)) * 64 + (ly & 7) * 8 + (x & 7)  # soa_index
        out = np.zeros((idx.size, abi.STATE_WORDS), dtype=np.uint32)
        out[:, :6] = w.reshape(6, -1)[:, idx].T
        return out

    def radiance_image(self) -> np.ndarray:
        return self.radiance.cpu().numpy().reshape(self.local_rows, self.width, 4)


class TiledRenderer:
    """Single-process multi-device tiling through librt_hip.so (rt_tiled_*): rank r renders the block-cyclic
    row bands b ≡ r (mod N) on devices[r] and copies them into their rows of the gathered frame (one strided
    peer copy per rank).  The C-ABI path a C++ viewer uses for the north star's 8-GPU split, without torch."""

    def __init__(self, width: int, height: int, devices, scene: Scene, band_rows: int = 16, rng: str = "xorwow",
                 seed: int = 1984):
        if not torch.cuda.is_available():
            raise RTError("no HIP device visible: librt_hip.so renders on MI355X only")
        self.width, self.height = width, height
        self.devices = list(devices)
        self._devs = (C.c_int * len(self.devices))(*self.devices)
        d = abi.TiledDesc(C.cast(self._devs, C.POINTER(C.c_int)), len(self.devices), band_rows, width, height,
                          abi.RT_FLAG_RNG_PHILOX if rng == "philox" else 0, 0, seed)
        self._scene_desc = scene.desc()
        self.handle = C.c_void_p()
        check(lib().rt_tiled_create(C.byref(d), C.byref(self._scene_desc), C.byref(self.handle)), "rt_tiled_create")
        self.pos = torch.zeros(width * height, dtype=torch.int32, device=torch.device("cuda", self.devices[0]))
        self.timing = abi.TiledTiming()

    def render(self, spp: int, max_depth: int, inputs: abi.InputStruct, flags: int = 0, frame: int | None = None,
               pos: torch.Tensor | None = None) -> torch.Tensor:
        """One frame over all ranks, gathered into `pos` (default: a buffer on devices[0]); synchronous."""
        out = self.pos if pos is None else pos
        f = abi.TiledFrame(out.data_ptr(), spp, max_depth, flags, frame or 0, 0 if frame is None else 1, 0, inputs)
        check(lib().rt_tiled_render(self.handle, C.byref(f), C.byref(self.timing)), "rt_tiled_render")
        return out

    def image(self) -> np.ndarray:
        return self.pos.cpu().numpy().view(np.uint32).reshape(self.height, self.width)

    def close(self) -> None:
        if self.handle:
            lib().rt_tiled_destroy(self.handle)
            self.handle = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
