"""Cost and worth of light sampling in rt_radiance_rays (RT_RADIANCE_DIRECT_LIGHT) on one GPU.

Time: per config (default c3, c2, c5) at 1920x1080, dense Philox camera rays of the whole frame (stream ids = pixel
indices, both outputs), the flagged and the flagless call at 1 and 4 samples alternating in one process on one stream,
each timed with HIP events; the median of --calls calls after --warmup, the ratio flagged / flagless with the quartiles
of the per-iteration ratios, and one untimed call of each for the rays traced.  c3 has a sampled light (the ceiling
lamp); c2 and c5 have none, so their flagged call launches the flagless kernel and must cost its time.

Worth (c3): the mean squared error of the flagged and the flagless mean at 1, 4 and 16 samples against the flagless mean
of 16384 samples on 32x32 centre rays at depth 8 (tests/test_gpu_direct_light.py's set-up; the estimates on another
rng_frame than the reference), and with the 1080p times the equal-time efficiency
(MSE_plain * t_plain) / (MSE_flag * t_flag): how many times longer the flagless call runs to the flagged one's error.
(The 16-sample time is taken as four times the 4-sample one.)

Prints one JSON line and writes it to --json.
"""
import argparse, ctypes as C, json, os, statistics, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from cudaraytracer_amd import abi, scenes
from cudaraytracer_amd._lib import check, lib
from cudaraytracer_amd.renderer import DeviceScene, camera_rays

ap = argparse.ArgumentParser()
ap.add_argument("--calls", type=int, default=30, help="timed calls (the median is reported)")
ap.add_argument("--warmup", type=int, default=5)
ap.add_argument("--width", type=int, default=1920)
ap.add_argument("--height", type=int, default=1080)
ap.add_argument("--configs", default="c3,c2,c5")
ap.add_argument("--texture", default="", help="WxH of config 5's images (default: the config's 8192x4096)")
ap.add_argument("--json", default="profiles/direct_light_bench.json")
args = ap.parse_args()
SEED = 1984
DIRECT = abi.RT_RADIANCE_DIRECT_LIGHT
device = torch.device("cuda", 0)


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


def radiance_call(ds, rays, index, outs, bg, k, depth, flags, frame=0, counters=None, rays_per_lane=0):
    a = abi.RadianceArgs()
    a.rays, a.stream_ids, a.sum, a.mean = rays.data_ptr(), index.data_ptr(), outs[0].data_ptr(), outs[1].data_ptr()
    a.n, a.samples_per_ray, a.max_depth, a.rng_seed, a.rng_frame = rays.shape[0], k, depth, SEED, frame
    a.flags, a.rays_per_lane = flags, rays_per_lane
    a.background_start[:], a.background_end[:] = list(bg[0]), list(bg[1])
    if counters is not None:
        a.counters = counters.data_ptr()
    stream = C.c_void_p(torch.cuda.current_stream(device).cuda_stream)
    return lambda: check(lib().rt_radiance_rays(ds.handle, C.byref(a), stream), "rt_radiance_rays")


def measure(name: str) -> dict:
    cfg = scenes.CONFIGS[name].scaled(args.width, args.height)
    if name == "c5" and args.texture:
        cfg.texture_size = tuple(int(v) for v in args.texture.split("x"))
    w, h, n = cfg.width, cfg.height, cfg.width * cfg.height
    inputs = cfg.inputs()
    scene = cfg.scene_desc()
    ds = DeviceScene(scene)
    bg = (tuple(inputs.background_start), tuple(inputs.background_end))
    out = {"config": name, "depth": cfg.depth, "rays_in_batch": n, "sampled_lights": scenes.scene_lights(scene)}
    rays, index = camera_rays(inputs, w, h, jitter="philox", sample=0, seed=SEED)
    outs = (torch.empty((n, 4), device=device), torch.empty((n, 4), device=device))
    for k in (1, 4):
        t_flag, t_plain = timed(radiance_call(ds, rays, index, outs, bg, k, cfg.depth, DIRECT),
                                radiance_call(ds, rays, index, outs, bg, k, cfg.depth, 0))
        torch.cuda.synchronize()
        m_flag, m_plain = statistics.median(t_flag), statistics.median(t_plain)
        case = {"flagged_ms": round(m_flag, 4), "flagless_ms": round(m_plain, 4), "ratio": round(m_flag / m_plain, 3),
                "ratio_quartiles": quartiles([a / b for a, b in zip(t_flag, t_plain)]),
                "flagged_ns_per_path": round(m_flag * 1e6 / (n * k), 3), "flagless_ns_per_path": round(m_plain * 1e6 / (n * k), 3)}
        for key, flags in (("flagged_rays", DIRECT), ("flagless_rays", 0)):  # one untimed call of each: the rays traced
            counters = torch.zeros(abi.COUNTERS_WORDS, dtype=torch.int64, device=device)
            radiance_call(ds, rays, index, outs, bg, k, cfg.depth, flags, counters=counters)()
            torch.cuda.synchronize()
            case[key] = int(counters[0].item())
        out[f"dense_{k}spp"] = case
    ds.close()
    return out


def cornell_error(times: dict) -> dict:
    """MSE of both estimators on c3 32 x 32 centre rays at depth 8 against 16384 flagless samples, and with `times`
    ({samples: (flagged ms, flagless ms)} at 1080p) the equal-time efficiency."""
    cfg = scenes.CONFIGS["c3"]
    inputs = cfg.inputs()
    ds = DeviceScene(cfg.scene_desc())
    bg = (tuple(inputs.background_start), tuple(inputs.background_end))
    rays, index = camera_rays(inputs, 32, 32)
    outs = (torch.empty((1024, 4), device=device), torch.empty((1024, 4), device=device))
    radiance_call(ds, rays, index, outs, bg, abi.PHILOX_MAX_SPP, 8, 0, frame=0, rays_per_lane=1)()
    torch.cuda.synchronize()
    ref = outs[1][:, :3].double().cpu().numpy()
    out = {}
    for k in (1, 4, 16):
        mse = {}
        for key, flags in (("flagged", DIRECT), ("flagless", 0)):
            # the mean over 8 independent estimates (rng_frame 7 .. 14) of the squared error: steadier than one
            errs = []
            for frame in range(7, 15):
                radiance_call(ds, rays, index, outs, bg, k, 8, flags, frame=frame, rays_per_lane=1)()
                torch.cuda.synchronize()
                errs.append(float(((outs[1][:, :3].double().cpu().numpy() - ref) ** 2).mean()))
            mse[key] = float(np.mean(errs))
        t_flag, t_plain = times[k]
        out[f"{k}spp"] = {"mse_flagged": mse["flagged"], "mse_flagless": mse["flagless"],
                          "mse_ratio": round(mse["flagged"] / mse["flagless"], 4),
                          "equal_time_efficiency": round(mse["flagless"] * t_plain / (mse["flagged"] * t_flag), 2)}
    ds.close()
    return out


results = [measure(c) for c in args.configs.split(",")]
out = {"workload": f"{args.width}x{args.height} Philox camera rays, rt_radiance_rays with and without RT_RADIANCE_DIRECT_LIGHT",
       "calls": args.calls, "warmup": args.warmup, "device": torch.cuda.get_device_name(0), "configs": results}
c3 = next((c for c in results if c["config"] == "c3"), None)
if c3 is not None:
    t1 = (c3["dense_1spp"]["flagged_ms"], c3["dense_1spp"]["flagless_ms"])
    t4 = (c3["dense_4spp"]["flagged_ms"], c3["dense_4spp"]["flagless_ms"])
    out["c3_error"] = cornell_error({1: t1, 4: t4, 16: (4 * t4[0], 4 * t4[1])})
line = json.dumps(out)
if args.json:
    os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
    with open(args.json, "w") as fh:
        fh.write(line + "\n")
print(line, flush=True)
