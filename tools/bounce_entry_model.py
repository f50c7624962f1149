"""CPU model of the bounce entries' saving on C2 (written before any timing): from the host-built tree of
the RTIOW scene, the node visits a bounce ray spends descending to the leaf its record starts at — a, the leaf's
ancestors — against the ⌈a/2⌉ chain visits that replace them, per origin class:
  * origins on a sphere: the sphere's own leaf (the grid cell of a surface point may name a neighbour; both printed);
  * origins on the visible ground: C2's camera rays that hit the ground sphere first, looked up through the grid.
No GPU.   python tools/bounce_entry_model.py
"""
from __future__ import annotations

import ctypes as C
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests"))

from cudaraytracer_amd import abi, scenes  # noqa: E402
from cudaraytracer_amd._lib import lib  # noqa: E402
import test_bounce_entry_host as tb  # noqa: E402  (the tables' reader and the host traversal)
from test_tile_entry_host import camera_rays  # noqa: E402

NONE = 0x7FFF


def ancestors(T, e):
    """a of a record: two per chain node behind the leaf, one for a direct sibling."""
    used = [int(r) for r in e[1:] if r != NONE]
    return sum(2 if T.info.num_nodes <= r < 0x8000 else 1 for r in used)


def cells(T, o):
    o32 = np.ascontiguousarray(o, np.float32)
    out = np.zeros(len(o32), np.uint32)
    assert lib().rt_bounce_entry_cells(C.byref(T.info), o32.ctypes.data_as(C.POINTER(C.c_float)), len(o32),
                                       out.ctypes.data_as(C.POINTER(C.c_uint32))) == 0
    return out


def main():
    cfg = scenes.CONFIGS["c2"]
    T = tb.tables("rtiow")  # C2's scene
    a_rec = np.array([ancestors(T, e) if e[0] != 0 else 0 for e in T.records])
    leaf_of = {int(e[0]): k for k, e in enumerate(T.records) if e[0] != 0}
    P = T.prims.astype(np.float64)
    ground = int(np.argmax(np.abs(P[:, 3])))
    rng = np.random.default_rng(3)
    print(f"tree: {T.info.num_nodes} nodes + {T.info.num_chain_nodes} chain nodes, depth {T.info.depth}, "
          f"{len(T.records)} leaves, grid {tuple(T.info.grid_dim)}; root records {int((T.records[:, 0] == 0).sum())}")

    def report(name, a):
        half = np.ceil(a / 2.0)
        print(f"{name}: mean a {a.mean():.2f} -> mean ceil(a/2) {half.mean():.2f}: {a.mean() - half.mean():.2f} visits fewer")
        return a.mean() - half.mean()

    # spheres: own leaf, and the leaf their surface points look up
    own = []
    for k in range(len(P)):
        if k == ground:
            continue
        for leaf, rec in leaf_of.items():
            l = leaf ^ 0xFFFF
            if (l >> 2) <= k <= (l >> 2) + (l & 3):
                own.append(a_rec[rec])
    s_own = report("sphere origins, own leaf", np.array(own, float))
    idx = rng.integers(0, len(P) - 1, 4000)
    idx = np.where(idx >= ground, idx + 1, idx)
    v = rng.normal(size=(len(idx), 3))
    pts = P[idx, 0:3] + P[idx, 3:4] * v / np.linalg.norm(v, axis=1)[:, None]
    s_grid = report("sphere origins, through the grid", a_rec[T.grid[cells(T, pts)]].astype(float))
    # the visible ground: C2's camera rays (pixel centres of a 192 x 108 grid) whose closest hit is the ground sphere
    w, h = 192, 108
    xs, gs = np.meshgrid(np.arange(w), np.arange(h))
    o, d = camera_rays(cfg.inputs(), w, h, xs.ravel(), gs.ravel(), 0.5, 0.5)
    o, d = o.astype(np.float64), d.astype(np.float64)
    t_all = tb.brute_force(T, o, d)
    t_g = tb._prim_t(np.broadcast_to(P[ground], (len(o), 8)), o, d, np.full(len(o), np.inf))
    vis = np.isfinite(t_g) & (t_g == t_all)
    gp = o[vis] + t_g[vis, None] * d[vis]
    g_grid = report(f"ground origins ({int(vis.sum())} visible points), through the grid", a_rec[T.grid[cells(T, gp)]].astype(float))
    g_own = report("ground origins, own leaf (no grid)", np.array([a_rec[rec] for leaf, rec in leaf_of.items()
                                                                    if (leaf ^ 0xFFFF) >> 2 <= ground <= ((leaf ^ 0xFFFF) >> 2) + ((leaf ^ 0xFFFF) & 3)], float))
    # what the host traversal counts for rays from those points (cosine-ish upward directions for the ground, any
    # outward direction for the spheres): visits from the record against visits from the root
    for name, org, nrm in (("ground", gp, (gp - P[ground, 0:3]) / np.abs(P[ground, 3])),
                           ("spheres", pts, (pts - P[idx, 0:3]) / P[idx, 3:4])):
        u = rng.normal(size=org.shape)
        u /= np.linalg.norm(u, axis=1)[:, None]
        dirs = nrm + u  # normal + a unit vector: the Lambertian scatter direction
        org32, dir32 = org.astype(np.float32).astype(np.float64), dirs.astype(np.float32).astype(np.float64)
        rec = T.records[T.grid[cells(T, org32)]]
        start = [[0] if e[0] == 0 else [int(r) for r in e if r != NONE] for e in rec]
        t1, v1 = tb.traverse(T, org32, dir32, start)
        t0, v0 = tb.traverse(T, org32, dir32, [[0]] * len(org32))
        assert np.array_equal(t0, t1)
        print(f"host traversal, Lambertian rays from {name}: {v0.mean():.2f} visits per ray from the root, {v1.mean():.2f} from the record")
    print(f"(saved per bounce ray with ground share g: g * {g_grid:.2f} + (1 - g) * {s_grid:.2f}; own-leaf-only ground: {g_own:.2f}, spheres {s_own:.2f})")


if __name__ == "__main__":
    main()
