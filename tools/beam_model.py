"""CPU model of the v3 kernels' per-tile entry records: no GPU needed.

Runs the library's own classifier (rt_tile_entries_host: csrc/rt_tile_entry.h, the function the device pre-pass runs)
over every 8x8 tile of a config's frame and prints what the tiles' beams touch — references and primitives per tile
with their histogram, the share of tiles that keep the root; once with every touched primitive and once with the
candidates hidden behind a covering sphere culled (rt_set_tile_occlusion, round 12) — then the §10 figures for the config: the bound from the camera rays' share of
the lane-visits, and the wave-level estimate from the counting build's numbers given on the command line.

    python tools/beam_model.py [--config c2] [--visits 11.08] [--camera-visits 10.0] [--prims 2.62]
"""
import argparse, ctypes as C, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
from cudaraytracer_amd import abi, scenes
from cudaraytracer_amd._lib import lib

ap = argparse.ArgumentParser()
ap.add_argument("--config", default="c2")
ap.add_argument("--visits", type=float, default=11.08, help="node visits per ray (counting build, tools/simd_eff.py)")
ap.add_argument("--camera-visits", type=float, default=10.0, help="node visits per camera ray")
ap.add_argument("--prims", type=float, default=2.62, help="primitive tests per ray")
ap.add_argument("--camera-prims", type=float, default=2.41, help="primitive tests per camera ray")
ap.add_argument("--node-share", type=float, default=0.69, help="node visits' share of the wave time")
ap.add_argument("--leaf-share", type=float, default=0.12)
ap.add_argument("--rays-per-pixel-sample", type=float, default=0.0, help="rays per camera ray (0: 417.86 M / 132.7 M)")
args = ap.parse_args()

cfg = scenes.CONFIGS[args.config]
sc = cfg.scene_desc() if args.config != "c5" else scenes.builtin(cfg.scene)
desc = sc.desc()
inputs = cfg.inputs()
t = abi.Tiling(cfg.height, 1, 0, cfg.height)
tiles_x, tiles_y = (cfg.width + 7) // 8, (cfg.height + 7) // 8
def tile_records(occlusion):
    """(tiles, 8) entries by the library's classifier, with rt_set_tile_occlusion at `occlusion`."""
    rec = np.zeros((tiles_x * tiles_y, 4), np.uint32)
    prev = lib().rt_set_tile_occlusion(occlusion)
    rc = lib().rt_tile_entries_host(C.byref(desc), C.byref(inputs), cfg.width, cfg.height, C.byref(t), 0, 0, len(rec),
                                    rec.ctypes.data_as(C.POINTER(C.c_uint32)))
    lib().rt_set_tile_occlusion(prev)
    if rc != 0:
        raise SystemExit(lib().rt_last_error().decode())
    return np.stack([rec & 0xFFFF, rec >> 16], axis=2).reshape(len(rec), 8)


print(f"{args.config}: {cfg.width}x{cfg.height}, {tiles_x * tiles_y} tiles; beam {8 + 2} x {8 + 2} px")
for occlusion in (0, 1):
    e = tile_records(occlusion)
    rooted = e[:, 0] == 0
    valid = (e != 0x7FFF) & ~rooted[:, None]
    refs = valid.sum(axis=1)[~rooted]
    prims = (((e ^ 0xFFFF) & 3) + 1)
    prims = np.where(valid, prims, 0).sum(axis=1)[~rooted]
    print(f" hidden candidates {'culled (rt_set_tile_occlusion 1, the default)' if occlusion else 'kept (rt_set_tile_occlusion 0)'}:")
    print(f"  tiles keeping the root: {rooted.sum()} ({100 * rooted.mean():.2f} %)")
    print(f"  references per tile: mean {refs.mean():.2f}, max {refs.max()}; <= 6: {100 * (refs <= 6).mean():.1f} %, <= 8: 100 %")
    print(f"  candidate primitives per tile: mean {prims.mean():.2f}, max {prims.max()}; tiles with 3 or more: {(prims >= 3).sum()}")
    print(f"  tiles by candidate primitives (0, 1, 2, ...): {np.bincount(prims).tolist()}")
    if not occlusion:
        prims_all = prims  # the round-8 figures below are for the records of every touched primitive

per_camera = args.rays_per_pixel_sample or 417.86 / 132.7
cam = 1.0 / per_camera
lane_visits = cam * args.camera_visits / args.visits
print(f"  camera rays: {100 * cam:.1f} % of the rays, {100 * lane_visits:.0f} % of the lane-visits")
print(f"  bound at unchanged lane efficiency: -{100 * lane_visits * args.node_share:.0f} % of the frame")
# wave level: a node iteration is saved only when no lane of the wave needs it.  The calls whose longest lanes were
# camera rays (taken as the camera rays' share of the rays) end about a third of a call earlier.
iters = cam / 3.0
extra_prims = (prims_all.mean() - args.camera_prims) * cam / args.prims
print(f"  wave-level estimate: node iterations -{100 * iters:.0f} % -> -{100 * iters * args.node_share:.1f} % of the frame; "
      f"primitive tests {'+' if extra_prims >= 0 else ''}{100 * extra_prims:.0f} % -> "
      f"{'+' if extra_prims >= 0 else ''}{100 * extra_prims * args.leaf_share:.1f} %; per-ray overhead +0.5 %")
print(f"  net: {100 * (-iters * args.node_share + extra_prims * args.leaf_share) + 0.5:+.1f} %")
