"""Cost of path-traced radiance per ray (rt_radiance_rays) and of the library's camera rays (rt_camera_rays) next to the
frame kernel they share their code with, on one GPU: BASELINE configs 2 (RTIOW) and 5 (textured spheres) at 1920x1080.

Per config, in one process and on one stream:
  camera     rt_camera_rays with RT_CAMERA_JITTER_PHILOX over the whole frame;
  dense      rt_radiance_rays at 1 and 4 samples on the whole frame's Philox camera rays (stream ids = pixel indices,
             both outputs; with the automatic rays per lane and with one) against rt_render of the same frame: variant 3,
             RT_FLAG_RNG_PHILOX, the same samples and depth, radiance plane only; one untimed counting call of each gives
             the box and primitive tests per ray.  The two calls alternate; `ratio` is radiance / render per ray (the same rays:
             both trace every path of the frame), with the quartiles of the per-iteration ratios as its spread.  The
             pixels whose mean differs from the frame's radiance are counted (the frame kernel replays ties through the
             reference BVH; the per-ray call returns the geometric closest hit);
  sparse     extra samples for a fixed pseudo-random 5 % of the pixels, listed in ascending order as a stream compaction
             would leave them: rt_camera_rays(pixels) + rt_radiance_rays(sum) + index_add_ of the sums into the frame's
             accumulation plane, against a second whole frame at 1 spp.

Each figure is the median of --calls calls after --warmup warm-up calls, timed with HIP events.  Prints one JSON line,
writes it to --json and a table to --text.
"""
import argparse, ctypes as C, json, os, statistics, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from cudaraytracer_amd import abi, scenes
from cudaraytracer_amd._lib import check, lib
from cudaraytracer_amd.renderer import DeviceScene, Renderer, camera_rays

ap = argparse.ArgumentParser()
ap.add_argument("--calls", type=int, default=30, help="timed calls (the median is reported)")
ap.add_argument("--warmup", type=int, default=5)
ap.add_argument("--width", type=int, default=1920)
ap.add_argument("--height", type=int, default=1080)
ap.add_argument("--configs", default="c2,c5")
ap.add_argument("--texture", default="", help="WxH of config 5's images (default: the config's 8192x4096)")
ap.add_argument("--share", type=float, default=0.05, help="share of the pixels the sparse case re-samples")
ap.add_argument("--json", default="profiles/r13a_radiance.json")
ap.add_argument("--text", default="profiles/r13a_radiance.txt")
args = ap.parse_args()
SEED = 1984
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


def measure(name: str) -> dict:
    cfg = scenes.CONFIGS[name].scaled(args.width, args.height)
    if name == "c5" and args.texture:
        cfg.texture_size = tuple(int(v) for v in args.texture.split("x"))
    w, h, n = cfg.width, cfg.height, cfg.width * cfg.height
    inputs = cfg.inputs()
    scene = cfg.scene_desc()
    ds = DeviceScene(scene)
    r = Renderer(w, h, rng="philox")
    r.render_init(SEED)
    bg = (tuple(inputs.background_start), tuple(inputs.background_end))
    out = {"config": name, "hittables": scene.num_hittables, "depth": cfg.depth, "rays_in_batch": n}
    (cam,) = timed(lambda: camera_rays(inputs, w, h, jitter="philox", sample=0, seed=SEED))
    out["camera_rays_ms"] = round(statistics.median(cam), 4)
    rays, index = camera_rays(inputs, w, h, jitter="philox", sample=0, seed=SEED)
    total, mean = torch.empty((n, 4), device=device), torch.empty((n, 4), device=device)
    stream = C.c_void_p(torch.cuda.current_stream(device).cuda_stream)

    def radiance_call(k: int, rays_per_lane: int = 0, counters: torch.Tensor | None = None):
        a = abi.RadianceArgs()
        a.rays, a.stream_ids, a.sum, a.mean = rays.data_ptr(), index.data_ptr(), total.data_ptr(), mean.data_ptr()
        a.n, a.samples_per_ray, a.max_depth, a.rng_seed, a.rays_per_lane = n, k, cfg.depth, SEED, rays_per_lane
        a.background_start[:], a.background_end[:] = list(bg[0]), list(bg[1])
        if counters is not None:
            a.counters, a.count_tests = counters.data_ptr(), 1
        return lambda: check(lib().rt_radiance_rays(ds.handle, C.byref(a), stream), "rt_radiance_rays")

    def per_ray(c) -> dict:
        rays_traced = max(1, int(c[0]))
        return {"rays": int(c[0]), "box_tests_per_ray": round(float(c[1]) / rays_traced, 2),
                "prim_tests_per_ray": round(float(c[2]) / rays_traced, 2)}

    for k in (1, 4):
        render = lambda: r.render(ds, k, cfg.depth, inputs, radiance=True, count=False, frame=0)
        case = {}
        for rpl in (0, 1):  # the automatic rays per lane (3 for this batch) and one ray per lane
            t_rad, t_ren = timed(radiance_call(k, rpl), render)
            torch.cuda.synchronize()
            m_rad, m_ren = statistics.median(t_rad), statistics.median(t_ren)
            case[f"rays_per_lane_{rpl}"] = {
                "radiance_ms": round(m_rad, 4), "render_ms": round(m_ren, 4), "ratio": round(m_rad / m_ren, 3),
                "ratio_quartiles": quartiles([a / b for a, b in zip(t_rad, t_ren)]),
                "radiance_ns_per_path": round(m_rad * 1e6 / (n * k), 3), "render_ns_per_path": round(m_ren * 1e6 / (n * k), 3)}
        if k == 1:  # sample 0 of the batch is the frame's own (at 4 spp a ray's later samples reuse its sample-0 camera ray)
            case["pixels_differing_from_the_frame"] = int((mean.view(h, w, 4) != r.radiance.view(h, w, 4)).any(dim=2).sum().item())
        # one untimed counting call of each: the traversal work per ray
        counters = torch.zeros(abi.COUNTERS_WORDS, dtype=torch.int64, device=device)
        radiance_call(k, 0, counters)()
        torch.cuda.synchronize()
        case["radiance_tests"] = per_ray(counters.cpu().numpy())
        r.counters.zero_()
        r.render(ds, k, cfg.depth, inputs, flags=abi.RT_FLAG_COUNT_TESTS, radiance=True, count=True, frame=0)
        torch.cuda.synchronize()
        case["render_tests"] = per_ray(r.counters.cpu().numpy())
        out[f"dense_{k}spp"] = case
    # sparse: a fixed pseudo-random share of the pixels, ascending
    g = torch.Generator(device="cpu")
    g.manual_seed(13)
    m = max(1, int(n * args.share))
    pick = torch.randperm(n, generator=g)[:m].sort().values.to(torch.int32).to(device)
    r.render(ds, 1, cfg.depth, inputs, flags=abi.RT_FLAG_ACCUMULATE, count=False, frame=0)
    accum = r.accum.view(n, 4)
    idx64 = pick.to(torch.int64)

    def resample():
        p_rays, p_index = camera_rays(inputs, w, h, pixels=pick, jitter="philox", sample=1, seed=SEED)
        accum.index_add_(0, idx64, ds.radiance(p_rays, samples=1, depth=cfg.depth, sample_base=1, stream_ids=p_index,
                                               seed=SEED, background=bg, mean=False))

    second = lambda: r.render(ds, 1, cfg.depth, inputs, radiance=True, count=False, frame=1)
    t_sp, t_fr = timed(resample, second)
    m_sp, m_fr = statistics.median(t_sp), statistics.median(t_fr)
    # ... and its three steps on their own (the list's rays kept): where the time of so small a batch goes
    p_rays, p_index = camera_rays(inputs, w, h, pixels=pick, jitter="philox", sample=1, seed=SEED)
    p_sum = torch.zeros((m, 4), device=device)
    t_cam, t_rad, t_add = timed(lambda: camera_rays(inputs, w, h, pixels=pick, jitter="philox", sample=1, seed=SEED),
                                lambda: ds.radiance(p_rays, samples=1, depth=cfg.depth, sample_base=1, stream_ids=p_index,
                                                    seed=SEED, background=bg, mean=False),
                                lambda: accum.index_add_(0, idx64, p_sum))
    out["sparse"] = {"pixels": m, "share": args.share, "resample_ms": round(m_sp, 4), "second_frame_ms": round(m_fr, 4),
                     "ratio": round(m_sp / m_fr, 3), "ratio_quartiles": quartiles([a / b for a, b in zip(t_sp, t_fr)]),
                     "resample_ns_per_path": round(m_sp * 1e6 / m, 3),
                     "steps_ms": {"camera_rays": round(statistics.median(t_cam), 4), "radiance": round(statistics.median(t_rad), 4),
                                  "index_add": round(statistics.median(t_add), 4)}}
    ds.close()
    return out


prev_variant = lib().rt_set_variant(3)
try:
    results = [measure(c) for c in args.configs.split(",")]
finally:
    lib().rt_set_variant(prev_variant)
out = {"workload": f"{args.width}x{args.height} Philox camera rays; rt_render: variant 3, RT_FLAG_RNG_PHILOX", "calls": args.calls,
       "warmup": args.warmup, "device": torch.cuda.get_device_name(0), "configs": results}
line = json.dumps(out)
rows = [f"# {out['workload']}; medians of {args.calls} calls after {args.warmup}, HIP events; {out['device']}",
        "# config  case        radiance_ms  render_ms  ratio  (quartiles)      ns/path radiance  render"]
for c in results:
    rows.append(f"{c['config']:7s}  camera_rays {c['camera_rays_ms']:10.4f}")
    for k in (1, 4):
        for rpl in (0, 1):
            d = c[f"dense_{k}spp"][f"rays_per_lane_{rpl}"]
            rows.append(f"{c['config']:7s}  dense {k} spp, rays per lane {'auto' if rpl == 0 else rpl:>4} {d['radiance_ms']:10.4f} {d['render_ms']:10.4f} "
                        f"{d['ratio']:6.3f}  {str(d['ratio_quartiles']):16s} {d['radiance_ns_per_path']:10.3f} {d['render_ns_per_path']:10.3f}")
        t, f = c[f"dense_{k}spp"]["radiance_tests"], c[f"dense_{k}spp"]["render_tests"]
        rows.append(f"{c['config']:7s}  dense {k} spp, box / primitive tests per ray: radiance {t['box_tests_per_ray']} / {t['prim_tests_per_ray']} "
                    f"({t['rays']} rays), render {f['box_tests_per_ray']} / {f['prim_tests_per_ray']} ({f['rays']} rays)")
    s = c["sparse"]
    rows.append(f"{c['config']:7s}  sparse {100 * s['share']:.0f} %  {s['resample_ms']:10.4f} {s['second_frame_ms']:10.4f} {s['ratio']:6.3f}  "
                f"{str(s['ratio_quartiles']):16s} {s['resample_ns_per_path']:10.3f}   ({s['pixels']} pixels against a whole second frame; "
                f"camera rays {s['steps_ms']['camera_rays']}, radiance {s['steps_ms']['radiance']}, index_add {s['steps_ms']['index_add']} ms alone)")
for path, text in ((args.json, line + "\n"), (args.text, "\n".join(rows) + "\n")):
    if path:
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
        with open(path, "w") as fh:
            fh.write(text)
print("\n".join(rows))
print(line, flush=True)
