"""Cost of the G-buffer pass and the denoiser next to the frame they serve: BASELINE config 5 (1920x1080, 1 spp, depth
4, textured spheres, moving camera, accumulation restarted every frame) on one GPU.

Times rt_render, rt_gbuffer and rt_denoise (N = 1, 3, 5; defaults otherwise; colour read from the accumulator,
RT_DENOISE_COLOR_IS_SUM, demodulated) separately with HIP events: warm-up frames, then the median over --frames frames
of the scripted camera orbit.  Prints one JSON line: ms, the compulsory bytes of each pass (per filter iteration one
colour plane read and one written and the normal/depth plane read, 16 B per pixel each; the first iteration also reads
prim_id, 4 B, and the albedo, 16 B; the last reads the albedo and writes the RGBA8 framebuffer, 4 B; the G-buffer pass
writes its 36 B per pixel) and the GB/s they amount to, and each pass's ratio to the render time of the same run.

`temporal` times rt_temporal in the same loop (colour from the accumulator, motion and RGBA8 outputs on, defaults
otherwise).  The camera really moves between frames (6 degrees of the orbit) and the G-buffer keeps the previous frame's
planes, so every call reprojects.  Its compulsory bytes per pixel: 36 of the current planes read, 36 of the previous
planes gathered (the four taps of neighbouring pixels overlap: about one plane set of unique bytes), 16 of history, 8 of
motion and 4 of RGBA8 written: 100.  `history_share` is the share of pixels that found history in the last frame.

`temporal_dynamic` times rt_temporal_dynamic in the same loop, on the same planes into the same output plane: one sphere
(hittable 4) is dragged back and forth, so every frame's scene is an rt_scene_edit of the one before and the motion
table of rt_scene_motion (uploaded outside the timed region) holds a non-identity entry.  rt_temporal on those frames
ignores the sphere's motion; its time is the yardstick (`ratio_to_temporal`).  The bytes are rt_temporal's: the table's
80 bytes stay in cache.  --dynamic-json writes the two entries to a file (profiles/temporal_dynamic_bench.json).

`temporal_moments` times rt_temporal_moments (without the table) in the same loop on the same planes, its moments planes
ping-ponging once per frame: rt_temporal's 100 bytes per pixel plus 8 of previous moments gathered and 8 written, 116.
`denoise_variance_n1/3/5` time rt_denoise_variance on that call's history and moments (defaults otherwise): the variance
stage reads 44 bytes per pixel and writes 16, each iteration reads the colour/variance and normal/depth planes and writes
one, the last also the RGBA8 framebuffer.  Both carry their ratios to rt_temporal and to rt_denoise (same N, and N = 3)
of the same run.  --variance-json writes these entries to a file (profiles/variance_bench.json).
"""
import argparse, json, os, statistics, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from cudaraytracer_amd import abi, scenes
from cudaraytracer_amd.renderer import DeviceScene, Renderer

ap = argparse.ArgumentParser()
ap.add_argument("--frames", type=int, default=120, help="timed frames (the median is reported)")
ap.add_argument("--warmup", type=int, default=12)
ap.add_argument("--width", type=int, default=0, help="override the config's size (with --height)")
ap.add_argument("--height", type=int, default=0)
ap.add_argument("--texture-size", default="", help="WxH of the three textures (default: the config's 8192x4096)")
ap.add_argument("--dynamic-json", default="", help="also write the temporal / temporal_dynamic entries to this file")
ap.add_argument("--variance-json", default="", help="also write the temporal_moments / denoise_variance entries to this file")
args = ap.parse_args()

cfg = scenes.CONFIGS["c5"]
if args.width and args.height:
    cfg = cfg.scaled(args.width, args.height)
if args.texture_size:
    cfg.texture_size = tuple(int(v) for v in args.texture_size.split("x"))
base_scene = cfg.scene_desc()
ds = DeviceScene(base_scene)
r = Renderer(cfg.width, cfg.height)


def dragged(frame: int):
    """The hittable list of `frame`: hittable 4 slides along a segment and back (12 steps each way)."""
    k = abs(frame % 24 - 12)
    h = type(base_scene.hittables).from_buffer_copy(base_scene.hittables)
    h[4].center[:] = [1.5 - 0.08 * k, 0.0, 2.5 + 0.03 * k]
    return h


r.render_init()
ITER = (1, 3, 5)
npix = cfg.width * cfg.height


def denoise_bytes(n: int) -> int:
    return npix * (n * 48 + 4 + 16 + 16 + 4)


def timed(fn) -> float:
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


times = {"render": [], "gbuffer": [], "temporal": [], "temporal_dynamic": [], "temporal_moments": [],
         **{f"denoise_n{n}": [] for n in ITER}, **{f"denoise_variance_n{n}": [] for n in ITER}}
total = args.warmup + args.frames
hittables = dragged(0)
history_share = {}
for f in range(total):
    pos, fwd = scenes.moving_camera(f % 60, 60)
    inp = scenes.camera_inputs(pos, fwd, cfg.fov)
    r.reset_accumulation()
    # the scene edit of this frame and its motion table, both outside the timed regions
    previous, hittables = hittables, dragged(f)
    ds, old = ds.edited(hittables), ds
    old.close()
    table = torch.from_numpy(scenes.scene_motion(previous, hittables)).to(r.device)
    torch.cuda.synchronize()
    t = {"render": timed(lambda: r.render(ds, cfg.spp, cfg.depth, inp, flags=abi.RT_FLAG_ACCUMULATE, count=False)),
         "gbuffer": timed(lambda: r.gbuffer(ds, inp, keep_previous=True))}
    # the three passes on the same planes; which of them runs first (and finds the caches cold) rotates by frame
    calls = {"temporal": lambda: r.temporal(source="accum", motion=True),
             "temporal_dynamic": lambda: r.temporal(source="accum", motion=True, prim_motion=table),
             "temporal_moments": lambda: r.temporal(source="accum", motion=True, moments=True)}
    names = ("temporal", "temporal_dynamic", "temporal_moments")
    order = names[f % 3:] + names[:f % 3]
    for i, name in enumerate(order):
        if i and r._history_spare is not None:  # (not the first frame) hand the planes back: a later call reads and
            r.history, r._history_spare = r._history_spare, r.history  # writes what the first did
        kept = (r.moments, r._moments_spare)
        t[name] = timed(calls[name])
        if name != "temporal_moments":  # (a call without moments drops the renderer's plane: the next frame needs it)
            r.moments, r._moments_spare = kept
        if f == total - 1:
            history_share[name] = float((r.history[..., 3] > 1.0).float().mean().item())
    for n in ITER:
        t[f"denoise_n{n}"] = timed(lambda: r.denoise_async(iterations=n, source="accum"))
        t[f"denoise_variance_n{n}"] = timed(lambda: r.denoise_variance_async(iterations=n))
    if f >= args.warmup:
        for k, v in t.items():
            times[k].append(v)

ms = {k: statistics.median(v) for k, v in times.items()}
out = {"config": "c5", "workload": f"{cfg.width}x{cfg.height}, {cfg.spp} spp, depth {cfg.depth}", "frames": args.frames,
       "warmup": args.warmup, "device": torch.cuda.get_device_name(0), "render_ms": round(ms["render"], 4)}
gb = npix * 36
out["gbuffer"] = {"ms": round(ms["gbuffer"], 4), "bytes": gb, "GB_per_s": round(gb / ms["gbuffer"] / 1e6, 1),
                  "ratio_to_render": round(ms["gbuffer"] / ms["render"], 3)}
tb = npix * 100
out["temporal"] = {"ms": round(ms["temporal"], 4), "bytes": tb, "GB_per_s": round(tb / ms["temporal"] / 1e6, 1),
                   "ratio_to_render": round(ms["temporal"] / ms["render"], 3), "history_share": round(history_share["temporal"], 3)}
out["temporal_dynamic"] = {"ms": round(ms["temporal_dynamic"], 4), "bytes": tb,
                           "GB_per_s": round(tb / ms["temporal_dynamic"] / 1e6, 1),
                           "ratio_to_render": round(ms["temporal_dynamic"] / ms["render"], 3),
                           "ratio_to_temporal": round(ms["temporal_dynamic"] / ms["temporal"], 3),
                           "history_share": round(history_share["temporal_dynamic"], 3),
                           "table": [round(float(v), 4) for v in table[4].tolist()]}
if args.dynamic_json:
    with open(args.dynamic_json, "w") as fh:
        json.dump({k: out[k] for k in ("config", "workload", "frames", "warmup", "device", "render_ms", "temporal",
                                        "temporal_dynamic")}, fh)
        fh.write("\n")
for n in ITER:
    m, b = ms[f"denoise_n{n}"], denoise_bytes(n)
    out[f"denoise_n{n}"] = {"ms": round(m, 4), "bytes": b, "GB_per_s": round(b / m / 1e6, 1),
                            "ms_per_iteration": round(m / n, 4), "ratio_to_render": round(m / ms["render"], 3)}
mb = npix * 116
out["temporal_moments"] = {"ms": round(ms["temporal_moments"], 4), "bytes": mb,
                           "GB_per_s": round(mb / ms["temporal_moments"] / 1e6, 1),
                           "ratio_to_render": round(ms["temporal_moments"] / ms["render"], 3),
                           "ratio_to_temporal": round(ms["temporal_moments"] / ms["temporal"], 3),
                           "ratio_to_denoise_n3": round(ms["temporal_moments"] / ms["denoise_n3"], 3),
                           "history_share": round(history_share["temporal_moments"], 3)}
for n in ITER:
    m, b = ms[f"denoise_variance_n{n}"], npix * (60 + 48 * n + 4)
    out[f"denoise_variance_n{n}"] = {"ms": round(m, 4), "bytes": b, "GB_per_s": round(b / m / 1e6, 1),
                                     "ratio_to_render": round(m / ms["render"], 3),
                                     "ratio_to_temporal": round(m / ms["temporal"], 3),
                                     "ratio_to_denoise_same_n": round(m / ms[f"denoise_n{n}"], 3),
                                     "ratio_to_denoise_n3": round(m / ms["denoise_n3"], 3)}
if args.variance_json:
    with open(args.variance_json, "w") as fh:
        keys = ("config", "workload", "frames", "warmup", "device", "render_ms", "temporal", "denoise_n1", "denoise_n3",
                "denoise_n5", "temporal_moments", "denoise_variance_n1", "denoise_variance_n3", "denoise_variance_n5")
        json.dump({k: out[k] for k in keys}, fh)
        fh.write("\n")
print(json.dumps(out), flush=True)
