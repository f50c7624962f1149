"""Cost of adaptive sampling on the device (rt_adaptive_select, rt_adaptive_samples) next to the three-step path it
replaces (rt_camera_rays + rt_radiance_rays + an addition, tools/bench_radiance.py's sparse case), on one GPU: BASELINE
configs 2 (RTIOW) and 5 (textured spheres) at 1920x1080, by tools/bench_radiance.py's protocol.

Per config, in one process and on one stream:
  sparse     the same fixed pseudo-random 5 % of the pixels as tools/bench_radiance.py, ascending, one extra sample each
             (sample 1 of frame 0) into the frame's accumulation plane: the fused pass (rt_adaptive_samples on the list,
             no device count) against the three steps with the list made by torch; the two alternate.  The fused pass
             alone into history and moments planes; the three steps alone; and rt_adaptive_select alone on the planes a
             reset rt_temporal_moments leaves (min_history 2: every hit pixel is listed, the longest list there is) and
             with an empty list (count only).
  orbit      (config 5 only) six 1-spp frames of the scripted orbit through gbuffer and rt_temporal_moments; tau is
             bisected (untimed) until about 5 % of the pixels are listed at max_samples 4; then select, the fused pass
             with the device count, and the two together are timed on those planes, which are restored before every
             call.  The list's k histogram is reported.

Each figure is the median of --calls calls after --warmup warm-up calls, timed with HIP events.  --quality adds the
small end-to-end sequence of tests/test_variance_host.py (config 5 at 64x48, 1 spp, depth 4, six frames, Philox streams):
the mean squared error of the history, and of the filtered history, against the oracle's 1024-spp radiance without
extra samples and, for a few (tau, min_history, lum_floor) triples, with the adaptive pass after every frame's temporal
pass and with the same number of extra paths per frame spread over pseudo-random pixels.  Prints one JSON line, writes
it to --json and a table to --text.
"""
import argparse, json, os, statistics, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch
from cudaraytracer_amd import abi, scenes
from cudaraytracer_amd._lib import lib
from cudaraytracer_amd.renderer import DeviceScene, Renderer, camera_rays

ap = argparse.ArgumentParser()
ap.add_argument("--calls", type=int, default=30, help="timed calls (the median is reported)")
ap.add_argument("--warmup", type=int, default=5)
ap.add_argument("--width", type=int, default=1920)
ap.add_argument("--height", type=int, default=1080)
ap.add_argument("--configs", default="c2,c5")
ap.add_argument("--texture", default="", help="WxH of config 5's images (default: the config's 8192x4096)")
ap.add_argument("--share", type=float, default=0.05, help="share of the pixels that get extra samples")
ap.add_argument("--quality", action="store_true", help="also the 64x48 sequence's error figures (needs the oracle)")
ap.add_argument("--json", default="profiles/r14a_adaptive.json")
ap.add_argument("--text", default="profiles/r14a_adaptive.txt")
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


def timed(*fns, prepare=None) -> list:
    """Per call the list of its timed durations (ms), the calls alternating; `prepare` runs untimed before each."""
    t = [[] for _ in fns]
    for i in range(args.warmup + args.calls):
        for k, fn in enumerate(fns):
            if prepare:
                prepare()
            t[k].append(one_call(fn))
    return [x[args.warmup:] for x in t]


def med(x) -> float:
    return round(statistics.median(x), 4)


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
    out = {"config": name, "hittables": scene.num_hittables, "depth": cfg.depth, "pixels": n}
    g = torch.Generator(device="cpu")
    g.manual_seed(13)
    m = max(1, int(n * args.share))
    pick = torch.randperm(n, generator=g)[:m].sort().values.to(torch.int32).to(device)
    idx64 = pick.to(torch.int64)
    r.render(ds, 1, cfg.depth, inputs, flags=abi.RT_FLAG_ACCUMULATE, radiance=True, count=False, frame=0)
    r.gbuffer(ds, inputs)
    r.temporal(moments=True)  # a reset pass: history (c, 1), moments (l, l·l)
    accum = r.accum.view(n, 4)
    fused = lambda: ds.adaptive_samples(pick, inputs, w, h, cfg.depth, accum=accum, sample_base=1, seed=SEED, frame=0)

    def three_steps():
        p_rays, p_index = camera_rays(inputs, w, h, pixels=pick, jitter="philox", sample=1, seed=SEED)
        accum.index_add_(0, idx64, ds.radiance(p_rays, samples=1, depth=cfg.depth, sample_base=1, stream_ids=p_index,
                                               seed=SEED, background=bg, mean=False))

    # the two give the same bits: checked once on a copy of the plane
    before = accum.clone()
    fused()
    mine = accum.clone()
    accum.copy_(before)
    three_steps()
    torch.cuda.synchronize()
    same = bool(torch.equal(mine, accum))
    t_f, t_3 = timed(fused, three_steps)
    m_f, m_3 = statistics.median(t_f), statistics.median(t_3)
    fused_hm = lambda: ds.adaptive_samples(pick, inputs, w, h, cfg.depth, history=r.history, moments=r.moments,
                                           sample_base=1, seed=SEED, frame=0)
    (t_hm,) = timed(fused_hm)
    r.temporal(moments=True, reset=True)
    select_all = lambda: r.adaptive_select(tau=1e6, min_history=2, max_samples=1)
    select_none = lambda: r.adaptive_select(tau=1e6, min_history=0, max_samples=1, capacity=0)
    (t_sa,) = timed(select_all)
    listed = int(r.adaptive_count.cpu()[0])
    (t_sn,) = timed(select_none)
    out["sparse"] = {"pixels": m, "share": args.share, "same_bits_as_three_steps": same,
                     "fused_ms": round(m_f, 4), "three_steps_ms": round(m_3, 4), "ratio": round(m_f / m_3, 3),
                     "ratio_quartiles": quartiles([a / b for a, b in zip(t_f, t_3)]),
                     "fused_history_moments_ms": med(t_hm), "fused_ns_per_path": round(m_f * 1e6 / m, 3),
                     "select_ms": med(t_sa), "select_listed": listed, "select_count_only_ms": med(t_sn)}
    if name == "c5":
        out["orbit"] = orbit(ds, cfg, w, h, n)
    ds.close()
    return out


def orbit(ds, cfg, w, h, n) -> dict:
    """Six frames of the scripted orbit, then the adaptive pass on the real planes with about `share` of the pixels listed."""
    r = Renderer(w, h, rng="philox")
    r.render_init(SEED)
    for k in range(6):
        pos, fwd = scenes.moving_camera(k, 360)
        inputs = scenes.camera_inputs(pos, fwd, cfg.fov)
        r.render(ds, 1, cfg.depth, inputs, radiance=True, count=False)
        r.gbuffer(ds, inputs, keep_previous=True)
        r.temporal(moments=True)
    torch.cuda.synchronize()
    params = dict(min_history=0, max_samples=4)
    lo, hi = 1e-3, 1e3  # the listed share falls in tau
    for _ in range(40):
        tau = (lo * hi) ** 0.5
        r.adaptive_select(tau=tau, capacity=0, **params)
        share = int(r.adaptive_count.cpu()[0]) / n
        if abs(share - args.share) < 0.002:
            break
        lo, hi = (tau, hi) if share > args.share else (lo, tau)
    hist0, mom0 = r.history.clone(), r.moments.clone()

    def restore():
        r.history.copy_(hist0)
        r.moments.copy_(mom0)

    pixels, samples, count = r.adaptive_select(tau=tau, **params)
    c = count.cpu().numpy()
    ks = samples[:int(c[0])].cpu().numpy()
    select = lambda: r.adaptive_select(tau=tau, **params)
    trace = lambda: ds.adaptive_samples(pixels, inputs, w, h, cfg.depth, samples=samples, count=count, history=r.history,
                                        moments=r.moments, max_samples=4, sample_base=1, seed=SEED, frame=5)
    both = lambda: r.adaptive(ds, inputs, cfg.depth, tau=tau, frame=5, seed=SEED, **params)
    t_s, t_t, t_b = timed(select, trace, both, prepare=restore)
    one = lambda: ds.adaptive_samples(pixels, inputs, w, h, cfg.depth, count=count, history=r.history, moments=r.moments,
                                      samples_per_pixel=1, max_samples=4, sample_base=1, seed=SEED, frame=5)
    (t_1,) = timed(one, prepare=restore)
    return {"tau": round(tau, 5), "listed": int(c[0]), "share": round(int(c[0]) / n, 4), "extra_paths": int(c[1]),
            "k_histogram": {str(k): int((ks == k).sum()) for k in (1, 2, 3, 4)},
            "select_ms": med(t_s), "fused_ms": med(t_t), "both_ms": med(t_b), "fused_k1_same_list_ms": med(t_1),
            "fused_over_k1": round(statistics.median(t_t) / statistics.median(t_1), 3)}


def quality() -> dict:
    """The 64x48 sequence of tests/test_variance_host.py on Philox streams: MSE of the filtered history against the
    oracle's 1024-spp radiance of the last frame, without extras, with the adaptive pass, and with as many extra paths
    per frame on pseudo-random pixels."""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from test_denoise_host import E2E_SIZE, end_to_end_frame, mse
    from test_temporal_host import SEQUENCE_FRAMES, sequence_inputs, sequence_reference
    e = end_to_end_frame()
    cfg, ref = e["cfg"], sequence_reference()
    w, h = E2E_SIZE
    n = w * h
    ds = DeviceScene(e["scene"])

    def run(mode: str, params=None, budget=None):
        r = Renderer(w, h, rng="philox")
        r.render_init(SEED)
        spent = []
        gen = np.random.default_rng(17)
        for k in range(SEQUENCE_FRAMES):
            inp = sequence_inputs(k)
            r.render(ds, 1, cfg.depth, inp, radiance=True)
            r.gbuffer(ds, inp, keep_previous=True)
            r.temporal(moments=True)
            if mode == "adaptive":
                spent.append(int(r.adaptive(ds, inp, cfg.depth, **params).cpu()[1]))
            elif mode == "uniform":
                total = budget[k]
                per = np.full(n, total // n, dtype=np.int32)
                per[gen.permutation(n)[:total % n]] += 1
                listed = np.nonzero(per)[0].astype(np.int32)
                if len(listed):
                    ds.adaptive_samples(torch.from_numpy(listed).to(device), inp, w, h, cfg.depth,
                                        samples=torch.from_numpy(per[listed]).to(device), history=r.history,
                                        moments=r.moments, max_samples=16, sample_base=1, seed=SEED, frame=k)
                spent.append(total)
        r.denoise_variance()
        torch.cuda.synchronize()
        return mse(r.denoised_variance.cpu().numpy(), ref), mse(r.history.cpu().numpy(), ref), spent

    plain = run("plain")
    runs = []
    # (lum_floor 1: below a luminance of 1 the rule bounds the absolute error, tau, instead of the relative one)
    for tau, min_history, lum_floor in ((0.25, 4, 0.01), (0.25, 0, 0.01), (0.5, 0, 0.01), (0.1, 0, 0.01), (0.25, 0, 1.0),
                                        (0.1, 0, 1.0), (0.05, 0, 1.0)):
        params = dict(tau=tau, min_history=min_history, max_samples=4, lum_floor=lum_floor)
        adaptive = run("adaptive", params)
        uniform = run("uniform", budget=adaptive[2])
        runs.append({"params": params, "extra_paths_per_frame": adaptive[2],
                     "mse_filtered": {"adaptive": round(adaptive[0], 5), "uniform": round(uniform[0], 5)},
                     "mse_history": {"adaptive": round(adaptive[1], 5), "uniform": round(uniform[1], 5)}})
    ds.close()
    return {"frame": f"c5 {w}x{h}, 1 spp, depth {cfg.depth}, {SEQUENCE_FRAMES} frames", "paths_per_frame": n,
            "no_extras": {"mse_filtered": round(plain[0], 5), "mse_history": round(plain[1], 5)}, "runs": runs}


prev_variant = lib().rt_set_variant(3)
try:
    results = [measure(c) for c in args.configs.split(",") if c]
    q = quality() if args.quality else None
finally:
    lib().rt_set_variant(prev_variant)
out = {"workload": f"{args.width}x{args.height}, Philox streams, extra samples of sample 1 on", "calls": args.calls,
       "warmup": args.warmup, "device": torch.cuda.get_device_name(0), "configs": results}
if q:
    out["quality"] = q
line = json.dumps(out)
rows = [f"# {out['workload']}; medians of {args.calls} calls after {args.warmup}, HIP events; {out['device']}"]
for c in results:
    s = c["sparse"]
    rows.append(f"{c['config']:4s} sparse {100 * s['share']:.0f} % ({s['pixels']} pixels, k = 1, into accum): fused {s['fused_ms']:.4f} ms, "
                f"three steps {s['three_steps_ms']:.4f} ms, ratio {s['ratio']:.3f} {s['ratio_quartiles']}, same bits: {s['same_bits_as_three_steps']}; "
                f"{s['fused_ns_per_path']} ns per path; into history + moments {s['fused_history_moments_ms']:.4f} ms")
    rows.append(f"{c['config']:4s} select: {s['select_ms']:.4f} ms listing {s['select_listed']} of {c['pixels']} pixels, "
                f"{s['select_count_only_ms']:.4f} ms with an empty list")
    if "orbit" in c:
        o = c["orbit"]
        rows.append(f"{c['config']:4s} orbit, tau {o['tau']}: {o['listed']} pixels listed ({100 * o['share']:.2f} %), {o['extra_paths']} paths, "
                    f"k histogram {o['k_histogram']}: select {o['select_ms']:.4f} ms, fused {o['fused_ms']:.4f} ms, both {o['both_ms']:.4f} ms; "
                    f"the same list at k = 1 {o['fused_k1_same_list_ms']:.4f} ms (ratio {o['fused_over_k1']})")
if q:
    rows.append(f"quality, {q['frame']} of {q['paths_per_frame']} paths; MSE against 1024 spp without extras: history {q['no_extras']['mse_history']}, "
                f"filtered {q['no_extras']['mse_filtered']}")
    for x in q["runs"]:
        rows.append(f"quality, {x['params']}: extra paths per frame {x['extra_paths_per_frame']}; MSE history {x['mse_history']}; "
                    f"MSE filtered {x['mse_filtered']}")
for path, text in ((args.json, line + "\n"), (args.text, "\n".join(rows) + "\n")):
    if path:
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
        with open(path, "w") as fh:
            fh.write(text)
print("\n".join(rows))
print(line, flush=True)
