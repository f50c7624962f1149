"""Cost of ray queries next to the passes they stand beside: rt_trace_rays, rt_query_rays (hits only, and all six
outputs) and rt_gbuffer on one GPU, first on BASELINE config 2 (the 488-sphere RTIOW scene, 16-bit BVH references), then
on sphere_field(9000, 6) (32-bit references) under the same camera.

The rays are the frame's 1920x1080 camera centre rays, written once by rt_camera_rays (Kernel.cu:130-146 with both jitter
numbers 0.5: rt_gbuffer's own rays), row-major: a wave's 64 consecutive rays are a 64-pixel piece of one row, where rt_gbuffer gives
a wave an 8x8 tile.  Each call is timed with HIP events on one stream: the median of --calls calls after --warmup
warm-up calls.  Bytes are the compulsory ones: 32 per ray read, plus the outputs written (hits 8; all outputs 16 + 16 +
4 + 8 + 4 + 8 = 56; rt_gbuffer reads no rays and writes 36).  Prints one JSON line and writes it to --json.
"""
import argparse, ctypes as C, json, os, statistics, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from cudaraytracer_amd import abi, scenes
from cudaraytracer_amd._lib import check, lib
from cudaraytracer_amd.renderer import DeviceScene, Renderer, camera_rays

ap = argparse.ArgumentParser()
ap.add_argument("--calls", type=int, default=50, help="timed calls (the median is reported)")
ap.add_argument("--warmup", type=int, default=5)
ap.add_argument("--width", type=int, default=0, help="override the config's size (with --height)")
ap.add_argument("--height", type=int, default=0)
ap.add_argument("--rays-per-lane", type=int, default=0)
ap.add_argument("--json", default="profiles/query_bench.json")
args = ap.parse_args()

cfg = scenes.CONFIGS["c2"]
if args.width and args.height:
    cfg = cfg.scaled(args.width, args.height)
inputs = cfg.inputs()
F = np.float32



def timed(fn) -> float:
    t = []
    for i in range(args.warmup + args.calls):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        t.append(e0.elapsed_time(e1))
    return statistics.median(t[args.warmup:])


r = Renderer(cfg.width, cfg.height)
n = cfg.width * cfg.height
rays, _ = camera_rays(inputs, cfg.width, cfg.height, device=r.device)  # jitter (0.5, 0.5): rt_gbuffer's rays, bit for bit
ALL = tuple(DeviceScene.QUERY_OUTPUTS)
bufs = {o: torch.zeros((n,) + shape, dtype=dtype, device=r.device) for o, (shape, dtype) in DeviceScene.QUERY_OUTPUTS.items()}


def query_call(ds: DeviceScene, names):
    a = abi.QueryArgs()
    a.rays, a.n, a.rays_per_lane = rays.data_ptr(), n, args.rays_per_lane
    for o in names:
        setattr(a, o, bufs[o].data_ptr())
    stream = C.c_void_p(r.stream())
    return lambda: check(lib().rt_query_rays(ds.handle, C.byref(a), stream), "rt_query_rays")


def measure(name: str, scene: scenes.Scene) -> dict:
    ds = DeviceScene(scene)
    stream = C.c_void_p(r.stream())
    hits = bufs["hits"]
    ms = {"trace_rays": timed(lambda: check(lib().rt_trace_rays(ds.handle, C.c_void_p(rays.data_ptr()), n,
                                                                 C.c_void_p(hits.data_ptr()), None, 0, stream), "rt_trace_rays")),
          "query_hits": timed(query_call(ds, ("hits",))),
          "query_all": timed(query_call(ds, ALL)),
          "gbuffer": timed(lambda: r.gbuffer(ds, inputs))}
    torch.cuda.synchronize()
    hit_share = float((bufs["hits"][:, 0] >= 0).float().mean().item())
    same = bool((bufs["prim_id"].reshape(cfg.height, cfg.width) == r.prim_id).float().mean().item() > 0.99)
    nbytes = {"trace_rays": n * 40, "query_hits": n * 40, "query_all": n * 88, "gbuffer": n * 36}
    out = {"scene": name, "hittables": scene.num_hittables, "hit_share": round(hit_share, 4), "pick_agrees_with_gbuffer": same}
    for k, v in ms.items():
        out[k] = {"ms": round(v, 4), "Mrays_per_s": round(n / v / 1e3, 1), "bytes": nbytes[k],
                  "GB_per_s": round(nbytes[k] / v / 1e6, 1), "ratio_to_trace_rays": round(v / ms["trace_rays"], 3)}
    ds.close()
    return out


out = {"workload": f"{cfg.width}x{cfg.height} camera centre rays of config c2's camera", "rays": n, "calls": args.calls,
       "warmup": args.warmup, "rays_per_lane": args.rays_per_lane, "device": torch.cuda.get_device_name(0),
       "c2": measure("c2 (RTIOW, 16-bit references)", scenes.builtin(cfg.scene)),
       "sphere_field": measure("sphere_field(9000, 6) (32-bit references)", scenes.sphere_field(9000, 6))}
line = json.dumps(out)
if args.json:
    os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
    with open(args.json, "w") as fh:
        fh.write(line + "\n")
print(line, flush=True)
