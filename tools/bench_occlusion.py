"""Cost of any-hit visibility queries (rt_occluded_rays) next to the closest-hit query they replace, on one GPU: first on
BASELINE config 2 (the 488-sphere RTIOW scene, 16-bit BVH references), then on sphere_field(9000, 6) (32-bit references)
under the same camera, 1920x1080.

Batch (a): the frame's camera centre rays (tools/bench_query.py's, written once by rt_camera_rays) with the range
(0.001, FLT_MAX): rt_occluded_rays with `occluded` only against rt_query_rays with `hits` only on the same buffer, with
the same rays_per_lane — automatic and 1 — the two calls alternating in one session.
Batch (b): shadow rays from the G-buffer's hit points (P = o + t·d with t from rt_query_rays' normal_depth) towards the
point light (2, 5, 3): d = L − P, range (0.001, 1); the camera's misses stay as they are with (0.001, FLT_MAX).  No
counterpart: its time and its tests per ray are reported.

Each call is timed with HIP events on one stream: the median of --calls calls after --warmup warm-up calls.  One untimed
count_tests call of each gives box and primitive tests per ray (rt_trace_rays' counters stand for the closest-hit
query: the same traversal at the automatic rays per lane).  Prints one JSON line and writes it to --json.
"""
import argparse, ctypes as C, json, os, statistics, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from cudaraytracer_amd import abi, scenes
from cudaraytracer_amd._lib import check, lib
from cudaraytracer_amd.renderer import DeviceScene, camera_rays

ap = argparse.ArgumentParser()
ap.add_argument("--calls", type=int, default=50, help="timed calls (the median is reported)")
ap.add_argument("--warmup", type=int, default=5)
ap.add_argument("--width", type=int, default=0, help="override the config's size (with --height)")
ap.add_argument("--height", type=int, default=0)
ap.add_argument("--json", default="profiles/occlusion_bench.json")
args = ap.parse_args()

cfg = scenes.CONFIGS["c2"]
if args.width and args.height:
    cfg = cfg.scaled(args.width, args.height)
inputs = cfg.inputs()
F = np.float32
FLT_MAX = float(np.finfo(F).max)
LIGHT = (2.0, 5.0, 3.0)



def one_call(fn) -> float:
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


def timed(*fns) -> list:
    """Medians (ms) of the given calls, alternating: call 0, call 1, ..., call 0, ..."""
    t = [[] for _ in fns]
    for i in range(args.warmup + args.calls):
        for k, fn in enumerate(fns):
            t[k].append(one_call(fn))
    return [statistics.median(x[args.warmup:]) for x in t]


device = torch.device("cuda", 0)
n = cfg.width * cfg.height
camera, _ = camera_rays(inputs, cfg.width, cfg.height, device=device)  # (origin, 0.001), (direction, FLT_MAX)
occ = torch.zeros(n, dtype=torch.uint8, device=device)
hits = torch.zeros((n, 2), dtype=torch.int32, device=device)
stream = C.c_void_p(torch.cuda.current_stream(device).cuda_stream)


def occlusion_call(ds: DeviceScene, rays: torch.Tensor, rays_per_lane: int, counters: torch.Tensor | None = None):
    a = abi.OcclusionArgs()
    a.rays, a.occluded, a.n, a.rays_per_lane = rays.data_ptr(), occ.data_ptr(), n, rays_per_lane
    if counters is not None:
        a.counters, a.count_tests = counters.data_ptr(), 1
    return lambda: check(lib().rt_occluded_rays(ds.handle, C.byref(a), stream), "rt_occluded_rays")


def query_call(ds: DeviceScene, rays: torch.Tensor, rays_per_lane: int):
    a = abi.QueryArgs()
    a.rays, a.hits, a.n, a.rays_per_lane = rays.data_ptr(), hits.data_ptr(), n, rays_per_lane
    return lambda: check(lib().rt_query_rays(ds.handle, C.byref(a), stream), "rt_query_rays")


def tests_per_ray(call_with_counters) -> dict:
    counters = torch.zeros(abi.COUNTERS_WORDS, dtype=torch.int64, device=device)
    call_with_counters(counters)()
    torch.cuda.synchronize()
    c = counters.cpu().numpy()
    rays = max(1, int(c[0]))
    return {"rays": int(c[0]), "box_tests_per_ray": round(float(c[1]) / rays, 2), "prim_tests_per_ray": round(float(c[2]) / rays, 2)}


def shadow_rays(ds: DeviceScene) -> torch.Tensor:
    """Batch (b), built on the device from rt_query_rays' normal_depth (float32 throughout)."""
    nd = ds.query(camera, outputs=("normal_depth",))["normal_depth"]
    hit = nd[:, 3] >= 0
    p = camera[:, 0, :3] + nd[:, 3:4] * camera[:, 1, :3]
    light = torch.tensor(LIGHT, dtype=torch.float32, device=device)
    rays = camera.clone()
    rays[:, 0, :3] = torch.where(hit[:, None], p, camera[:, 0, :3])
    rays[:, 1, :3] = torch.where(hit[:, None], light[None, :] - p, camera[:, 1, :3])
    rays[:, 1, 3] = torch.where(hit, torch.ones_like(nd[:, 3]), torch.full_like(nd[:, 3], FLT_MAX))
    return rays.contiguous()


def measure(name: str, scene: scenes.Scene) -> dict:
    ds = DeviceScene(scene)
    out = {"scene": name, "hittables": scene.num_hittables}
    for rpl in (0, 1):
        o_ms, q_ms = timed(occlusion_call(ds, camera, rpl), query_call(ds, camera, rpl))
        torch.cuda.synchronize()
        agree = bool(((occ != 0) == (hits[:, 0] >= 0)).all().item())
        out[f"camera_rays_per_lane_{rpl}"] = {
            "occluded_ms": round(o_ms, 4), "query_hits_ms": round(q_ms, 4), "ratio": round(o_ms / q_ms, 3),
            "occluded_Mrays_per_s": round(n / o_ms / 1e3, 1), "occluded_share": round(float((occ != 0).float().mean().item()), 4),
            "agrees_with_query_hits": agree}
    out["camera_tests"] = {"occluded": tests_per_ray(lambda c: occlusion_call(ds, camera, 0, c))}
    counters = torch.zeros(abi.COUNTERS_WORDS, dtype=torch.int64, device=device)
    check(lib().rt_trace_rays(ds.handle, C.c_void_p(camera.data_ptr()), n, C.c_void_p(hits.data_ptr()),
                              C.c_void_p(counters.data_ptr()), 1, stream), "rt_trace_rays")
    torch.cuda.synchronize()
    c = counters.cpu().numpy()
    out["camera_tests"]["closest_hit"] = {"rays": int(c[0]), "box_tests_per_ray": round(float(c[1]) / n, 2),
                                          "prim_tests_per_ray": round(float(c[2]) / n, 2)}
    shadow = shadow_rays(ds)
    for rpl in (0, 1):
        (s_ms,) = timed(occlusion_call(ds, shadow, rpl))
        torch.cuda.synchronize()
        out[f"shadow_rays_per_lane_{rpl}"] = {"occluded_ms": round(s_ms, 4), "occluded_Mrays_per_s": round(n / s_ms / 1e3, 1),
                                              "occluded_share": round(float((occ != 0).float().mean().item()), 4)}
    out["shadow_tests"] = tests_per_ray(lambda c: occlusion_call(ds, shadow, 0, c))
    ds.close()
    return out


out = {"workload": f"{cfg.width}x{cfg.height} camera centre rays of config c2's camera, and shadow rays from their hit points "
                   f"towards {LIGHT}", "rays": n, "calls": args.calls, "warmup": args.warmup,
       "device": torch.cuda.get_device_name(0),
       "c2": measure("c2 (RTIOW, 16-bit references)", scenes.builtin(cfg.scene)),
       "sphere_field": measure("sphere_field(9000, 6) (32-bit references)", scenes.sphere_field(9000, 6))}
line = json.dumps(out)
if args.json:
    os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
    with open(args.json, "w") as fh:
        fh.write(line + "\n")
print(line, flush=True)
