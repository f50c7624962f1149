"""Cost of the temporal-gradient passes (rt_temporal_gradient, rt_history_adapt) next to a whole 1-spp Philox rt_render
of the same scene, on one GPU: BASELINE configs 2 (RTIOW) and 5 (textured spheres) at 1920x1080, by
tools/bench_radiance.py's protocol.

Per config, in one process and on one stream: a 1-spp Philox frame with its radiance plane, a G-buffer and a reset
temporal pass (the history plane); one sphere is then moved by +0.3 in x (config 2: hittable 487, config 5: hittable 2)
and, in the edited scene, rt_temporal_gradient of that frame and rt_history_adapt on its plane are timed at stride 1, 3
and 8 (radius 1, power 4), alternating with a whole 1-spp Philox rt_render of the edited scene, which is the comparator:
there is no such pass to compare with.  rt_history_adapt rewrites the lengths in place; its cost does not depend on
their values.  Each figure is the median of --calls calls after --warmup warm-up calls, timed with HIP events.  Prints
one JSON line, writes it to --json and a table to --text.
"""
import argparse, json, os, statistics, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
from cudaraytracer_amd import abi, scenes
from cudaraytracer_amd._lib import check, lib
from cudaraytracer_amd.renderer import DeviceScene, Renderer
import ctypes as C

ap = argparse.ArgumentParser()
ap.add_argument("--calls", type=int, default=30, help="timed calls (the median is reported)")
ap.add_argument("--warmup", type=int, default=5)
ap.add_argument("--width", type=int, default=1920)
ap.add_argument("--height", type=int, default=1080)
ap.add_argument("--configs", default="c2,c5")
ap.add_argument("--texture", default="", help="WxH of config 5's images (default: the config's 8192x4096)")
ap.add_argument("--json", default="profiles/gradient_bench.json")
ap.add_argument("--text", default="profiles/gradient_bench.txt")
args = ap.parse_args()
SEED = 1984
MOVED = {"c2": 487, "c5": 2}
STRIDES = (1, 3, 8)


def one_call(fn) -> float:
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


def timed(*fns) -> list:
    """Per call the list of its timed durations (ms), the calls alternating."""
    t = [[] for _ in fns]
    for i in range(args.warmup + args.calls):
        for k, fn in enumerate(fns):
            t[k].append(one_call(fn))
    return [x[args.warmup:] for x in t]


def med(x) -> float:
    return round(statistics.median(x), 4)


def measure(name: str) -> dict:
    cfg = scenes.CONFIGS[name].scaled(args.width, args.height)
    if name == "c5" and args.texture:
        cfg.texture_size = tuple(int(v) for v in args.texture.split("x"))
    w, h, n = cfg.width, cfg.height, cfg.width * cfg.height
    inputs = cfg.inputs()
    scene = cfg.scene_desc()
    moved = scenes.Scene.from_bytes(scene.hittables_bytes(), scene.materials_bytes(), scene.images)
    moved.hittables[MOVED[name]].center[0] += 0.3
    ds, ds_b = DeviceScene(scene), DeviceScene(moved)
    print(f"{name}: scenes uploaded", flush=True)
    r = Renderer(w, h, rng="philox")
    r.render_init(SEED)
    r.render(ds, 1, cfg.depth, inputs, radiance=True, count=False, frame=0)
    r.gbuffer(ds, inputs)
    r.temporal()  # a reset pass: history (c, 1)
    other = Renderer(w, h, rng="philox")  # the comparator's planes: r's radiance stays the previous frame's
    other.render_init(SEED)
    frame = lambda: other.render(ds_b, 1, cfg.depth, inputs, radiance=True, count=False, frame=1)
    planes, fns, labels = {}, [frame], ["render_1spp_ms"]
    for s in STRIDES:
        planes[s] = ds_b.temporal_gradient(r.radiance, inputs, w, h, cfg.depth, stride=s, seed=SEED, frame=0)

        def grad(s=s):
            ds_b.temporal_gradient(r.radiance, inputs, w, h, cfg.depth, stride=s, seed=SEED, frame=0, gradient=planes[s])

        def adapt(s=s):
            a = abi.HistoryAdaptArgs()
            a.gradient, a.history = planes[s].data_ptr(), r.history.data_ptr()
            a.width, a.height, a.stride, a.radius, a.power, a.gain, a.lum_floor = w, h, s, 1, 4, 1.0, 0.01
            a.tiling = r.tiling()
            check(lib().rt_history_adapt(C.byref(a), C.c_void_p(r.stream())), "rt_history_adapt")

        fns += [grad, adapt]
        labels += [f"gradient_stride{s}_ms", f"adapt_stride{s}_ms"]
    torch.cuda.synchronize()
    out = {"config": name, "hittables": scene.num_hittables, "depth": cfg.depth, "pixels": n, "moved_hittable": MOVED[name]}
    for s in STRIDES:
        out[f"strata_stride{s}"] = int(planes[s].shape[0] * planes[s].shape[1])
        out[f"strata_with_gradient_stride{s}"] = round(float((planes[s][..., 0] > 0).float().mean().item()), 4)
    # the same call on the unedited scene: an exact zero everywhere
    zero = ds.temporal_gradient(r.radiance, inputs, w, h, cfg.depth, stride=1, seed=SEED, frame=0)
    out["unedited_strata_with_gradient"] = int((zero[..., 0] != 0).sum().item())
    print(f"{name}: timing", flush=True)
    times = timed(*fns)
    for label, t in zip(labels, times):
        out[label] = med(t)
    for s in STRIDES:
        both = [a + b for a, b in zip(times[labels.index(f"gradient_stride{s}_ms")], times[labels.index(f"adapt_stride{s}_ms")])]
        out[f"both_stride{s}_ms"] = med(both)
        out[f"both_over_render_stride{s}"] = round(statistics.median(b / f for b, f in zip(both, times[0])), 3)
    ds.close()
    ds_b.close()
    return out


results = [measure(c) for c in args.configs.split(",")]
line = json.dumps({"bench": "gradient", "width": args.width, "height": args.height, "calls": args.calls, "results": results})
print(line)
os.makedirs(os.path.dirname(os.path.join(ROOT, args.json)) or ".", exist_ok=True)
with open(os.path.join(ROOT, args.json), "w") as f:
    f.write(line + "\n")
rows = ["temporal gradient passes, %dx%d, median of %d calls after %d (ms)" % (args.width, args.height, args.calls, args.warmup)]
for r in results:
    rows.append(f"{r['config']}: 1-spp Philox rt_render {r['render_1spp_ms']}; "
                f"strata with a gradient on the unedited scene: {r['unedited_strata_with_gradient']}")
    for s in STRIDES:
        rows.append(f"  stride {s}: {r[f'strata_stride{s}']} strata ({r[f'strata_with_gradient_stride{s}']:.3f} with a gradient): "
                    f"rt_temporal_gradient {r[f'gradient_stride{s}_ms']}, rt_history_adapt {r[f'adapt_stride{s}_ms']}, "
                    f"both {r[f'both_stride{s}_ms']} = {r[f'both_over_render_stride{s}']} of the frame")
with open(os.path.join(ROOT, args.text), "w") as f:
    f.write("\n".join(rows) + "\n")
print("\n".join(rows))
