"""Cost of light sampling (RT_RADIANCE_DIRECT_LIGHT) in the fused frame passes on one GPU.

Per config (default c3, c2, c5) at 1920x1080, at the config's depth, all variants alternating in one process on one
stream, each call timed with HIP events; the median of --calls calls after --warmup, and for every ratio the quartiles of
the per-iteration ratios:

(a) a dense one-sample frame into an accumulation plane (every pixel listed in ascending order, sample 0):
    fused_flagged   rt_adaptive_samples with the flag,
    three_step      rt_camera_rays (the listed pixels, Philox jitter) + rt_radiance_rays with the flag (sum) + the addition
                    into the plane — the path that existed before,
    fused_flagless  rt_adaptive_samples without the flag;
(b) rt_temporal_gradient at stride 3 (all three outputs), flagged against flagless.

c3 has a sampled light (the ceiling lamp); c2 and c5 have none, so their flagged calls launch the flagless kernels and
must cost their time.  One untimed call of each variant gives the rays traced.  The comparators are the calls that were
there before, in the same run.

Prints one JSON line and writes it to --json.
"""
import argparse, ctypes as C, json, os, statistics, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from cudaraytracer_amd import abi, scenes
from cudaraytracer_amd._lib import check, lib
from cudaraytracer_amd.renderer import DeviceScene

ap = argparse.ArgumentParser()
ap.add_argument("--calls", type=int, default=30, help="timed calls (the median is reported)")
ap.add_argument("--warmup", type=int, default=5)
ap.add_argument("--width", type=int, default=1920)
ap.add_argument("--height", type=int, default=1080)
ap.add_argument("--configs", default="c3,c2,c5")
ap.add_argument("--stride", type=int, default=3)
ap.add_argument("--texture", default="", help="WxH of config 5's images (default: the config's 8192x4096)")
ap.add_argument("--json", default="profiles/direct_frame_bench.json")
args = ap.parse_args()
SEED = 1984
DIRECT = abi.RT_RADIANCE_DIRECT_LIGHT
device = torch.device("cuda", 0)


def stream() -> C.c_void_p:
    return C.c_void_p(torch.cuda.current_stream(device).cuda_stream)


def one_call(fn) -> float:
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


def timed(*fns) -> list:
    """Per call the list of its timed durations (ms), the calls alternating: call 0, call 1, ..., call 0, ..."""
    t = [[] for _ in fns]
    for i in range(args.warmup + args.calls):
        for k, fn in enumerate(fns):
            t[k].append(one_call(fn))
    return [x[args.warmup:] for x in t]


def quartiles(x) -> tuple:
    q = statistics.quantiles(x, n=4)
    return round(q[0], 3), round(q[2], 3)


def ratio(a: list, b: list) -> dict:
    return {"ratio": round(statistics.median(a) / statistics.median(b), 3),
            "ratio_quartiles": quartiles([x / y for x, y in zip(a, b)])}


def fused_call(ds, inputs, w, h, depth, pixels, accum, flags, counters=None):
    a = abi.AdaptiveSamplesArgs()
    a.pixels, a.accum = pixels.data_ptr(), accum.data_ptr()
    a.capacity, a.width, a.height = pixels.shape[0], w, h
    a.samples_per_pixel, a.max_samples, a.sample_base, a.max_depth, a.max_history = 1, 16, 0, depth, 32
    a.flags, a.rng_seed, a.rng_frame = flags, SEED, 0
    a.inputs = inputs
    if counters is not None:
        a.counters = counters.data_ptr()
    return lambda: check(lib().rt_adaptive_samples(ds.handle, C.byref(a), stream()), "rt_adaptive_samples")


def three_step_call(ds, inputs, w, h, depth, pixels, accum, rays, index, total, flags, counters=None):
    n = pixels.shape[0]
    c = abi.CameraRaysArgs()
    c.rays, c.pixel_index, c.pixels = rays.data_ptr(), index.data_ptr(), pixels.data_ptr()
    c.n, c.width, c.height, c.tiling, c.inputs = n, w, h, abi.Tiling(h, 1, 0, h), inputs
    c.flags, c.sample, c.rng_seed, c.rng_frame = abi.RT_CAMERA_JITTER_PHILOX, 0, SEED, 0
    r = abi.RadianceArgs()
    r.rays, r.stream_ids, r.sum = rays.data_ptr(), index.data_ptr(), total.data_ptr()
    r.n, r.samples_per_ray, r.sample_base, r.max_depth, r.rng_seed, r.rng_frame = n, 1, 0, depth, SEED, 0
    r.flags = flags
    r.background_start[:], r.background_end[:] = list(inputs.background_start), list(inputs.background_end)
    if counters is not None:
        r.counters = counters.data_ptr()

    def run():
        check(lib().rt_camera_rays(C.byref(c), stream()), "rt_camera_rays")
        check(lib().rt_radiance_rays(ds.handle, C.byref(r), stream()), "rt_radiance_rays")
        accum.add_(total)  # (dense and ascending: the plane's rows are the batch's)
    return run


def gradient_call(ds, inputs, w, h, depth, prev, outs, flags, counters=None):
    a = abi.TemporalGradientArgs()
    a.prev_color, a.gradient, a.resample, a.pixel = prev.data_ptr(), outs[0].data_ptr(), outs[1].data_ptr(), outs[2].data_ptr()
    a.width, a.height, a.stride, a.offset_x, a.offset_y = w, h, args.stride, 0, 0
    a.samples_per_pixel, a.max_depth, a.flags, a.rng_seed, a.rng_frame = 1, depth, flags, SEED, 0
    a.tiling = abi.Tiling(h, 1, 0, h)
    a.inputs = inputs
    if counters is not None:
        a.counters = counters.data_ptr()
    return lambda: check(lib().rt_temporal_gradient(ds.handle, C.byref(a), stream()), "rt_temporal_gradient")


def rays_of(make) -> int:
    counters = torch.zeros(abi.COUNTERS_WORDS, dtype=torch.int64, device=device)
    make(counters)()
    torch.cuda.synchronize()
    return int(counters[0].item())


def measure(name: str) -> dict:
    cfg = scenes.CONFIGS[name].scaled(args.width, args.height)
    if name == "c5" and args.texture:
        cfg.texture_size = tuple(int(v) for v in args.texture.split("x"))
    w, h, n = cfg.width, cfg.height, cfg.width * cfg.height
    inputs = cfg.inputs()
    scene = cfg.scene_desc()
    ds = DeviceScene(scene)
    out = {"config": name, "depth": cfg.depth, "pixels": n, "sampled_lights": scenes.scene_lights(scene)}
    pixels = torch.arange(n, dtype=torch.int32, device=device)
    accum = torch.zeros((n, 4), device=device)
    rays = torch.empty((n, 2, 4), device=device)
    index = torch.empty((n,), dtype=torch.int32, device=device)
    total = torch.empty((n, 4), device=device)
    fused = lambda flags: (lambda counters=None: fused_call(ds, inputs, w, h, cfg.depth, pixels, accum, flags, counters))  # noqa: E731
    steps = lambda counters=None: three_step_call(ds, inputs, w, h, cfg.depth, pixels, accum, rays, index, total, DIRECT, counters)  # noqa: E731
    t_fused, t_steps, t_plain = timed(fused(DIRECT)(), steps(), fused(0)())
    torch.cuda.synchronize()
    out["dense_1spp"] = {"fused_flagged_ms": round(statistics.median(t_fused), 4),
                         "three_step_flagged_ms": round(statistics.median(t_steps), 4),
                         "fused_flagless_ms": round(statistics.median(t_plain), 4),
                         "fused_over_three_step": ratio(t_fused, t_steps),
                         "flagged_over_flagless": ratio(t_fused, t_plain),
                         "fused_flagged_rays": rays_of(fused(DIRECT)), "three_step_rays": rays_of(steps),
                         "fused_flagless_rays": rays_of(fused(0))}
    sw, sh = -(-w // args.stride), -(-h // args.stride)
    prev = torch.zeros((n, 4), device=device)
    outs = (torch.empty((sw * sh, 2), device=device), torch.empty((sw * sh, 4), device=device),
            torch.empty((sw * sh,), dtype=torch.int32, device=device))
    grad = lambda flags: (lambda counters=None: gradient_call(ds, inputs, w, h, cfg.depth, prev, outs, flags, counters))  # noqa: E731
    t_flag, t_plain = timed(grad(DIRECT)(), grad(0)())
    torch.cuda.synchronize()
    out[f"gradient_stride{args.stride}"] = {"strata": sw * sh, "flagged_ms": round(statistics.median(t_flag), 4),
                                           "flagless_ms": round(statistics.median(t_plain), 4),
                                           "flagged_over_flagless": ratio(t_flag, t_plain),
                                           "flagged_rays": rays_of(grad(DIRECT)), "flagless_rays": rays_of(grad(0))}
    ds.close()
    return out


results = [measure(c) for c in args.configs.split(",")]
out = {"workload": f"{args.width}x{args.height}: rt_adaptive_samples (dense, 1 sample, accum) and rt_temporal_gradient "
                   f"(stride {args.stride}) with and without RT_RADIANCE_DIRECT_LIGHT; three steps = rt_camera_rays + "
                   "rt_radiance_rays with the flag + the addition",
       "calls": args.calls, "warmup": args.warmup, "device": torch.cuda.get_device_name(0), "configs": results}
line = json.dumps(out)
if args.json:
    os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
    with open(args.json, "w") as fh:
        fh.write(line + "\n")
print(line, flush=True)
