"""Where v3's node-uniform visits occur and how often the exactness check reaches stage 2, from the COUNT_TESTS
counters 18-23 (render.hip flush_counts): node iterations by active-lane count and the uniform ones of each class,
uniform iterations before / after the first divergent iteration of their v3_traverse call, stage-2 entries and
failures of bvh_clear and the shading passes with one.
    python tools/visit_uniformity.py [config = c2] [variant = 3]"""
import os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from cudaraytracer_amd import abi, scenes
from cudaraytracer_amd._lib import lib
from cudaraytracer_amd.renderer import DeviceScene, Renderer


def split(w):
    return w & 0xffffffff, (w >> 32) & 0xffffffff


cfg = scenes.CONFIGS[sys.argv[1] if len(sys.argv) > 1 else "c2"]
ds = DeviceScene(scenes.builtin(cfg.scene))
r = Renderer(cfg.width, cfg.height, rng=os.environ.get("RT_RNG", "xorwow"))
r.render_init()
lib().rt_set_variant(int(sys.argv[2]) if len(sys.argv) > 2 else 3)
r.counters.zero_()
r.render(ds, cfg.spp, cfg.depth, cfg.inputs(), flags=abi.RT_FLAG_COUNT_TESTS | abi.RT_FLAG_NO_STATE_WRITEBACK)
torch.cuda.synchronize()
c = [int(x) for x in r.counters.tolist()]
c = [x & 0xffffffffffffffff for x in c]
rays, wn, wshade, wuni, replays = c[0], c[4], c[6], c[11], c[17]
vis1, s2_fail = split(c[18])
cls = [("1", vis1, vis1)] + [(n, *split(c[i])) for n, i in (("2-4", 19), ("5-16", 20), ("17-64", 21))]
pre, post = split(c[22])
s2_enter, s2_pass = split(c[23])
print(f"{sys.argv[1] if len(sys.argv) > 1 else 'c2'}: rays {rays}, node iterations {wn}, uniform {wuni} ({wuni / max(1, wn):.4f})")
print("active lanes | node iterations | share | uniform | uniform share of class | share of all uniform")
for n, tot, uni in cls:
    print(f"{n:>12} | {tot:15d} | {tot / max(1, wn):.4f} | {uni:11d} | {uni / max(1, tot):.4f} | {uni / max(1, wuni):.4f}")
print(f"uniform iterations before the call's first divergent iteration: {pre} ({pre / max(1, wuni):.4f}), after: {post} "
      f"({post / max(1, wuni):.4f})")
print(f"shading passes {wshade} ({rays / max(1, wshade):.1f} lanes each); stage-2 entries {s2_enter} "
      f"({s2_enter / max(1, rays):.5f} per ray), stage-2 failures {s2_fail}, replays {replays}; passes with a stage-2 "
      f"entry {s2_pass} ({s2_pass / max(1, wshade):.4f})")
