"""CPU model of the bounce entries' direction classes on C2 (written before any timing): from the
library's own tables (rt_bounce_entries_host, rt_bounce_class_entries_host) the chain references a Lambertian bounce
ray (n + a point of the unit ball) starts with — the full record against the record of its direction class in form 1
(existing pairs) and form 2 (re-paired) — and the node visits of the host traversal from each, per origin class:
  * the visible ground: C2's camera rays that hit the ground sphere first, as tools/bounce_entry_model.py takes them;
  * sphere surfaces (upper halves).
No GPU.   python tools/bounce_class_model.py
"""
from __future__ import annotations

import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests"))

from cudaraytracer_amd import scenes  # noqa: E402
import test_bounce_entry_host as tb  # noqa: E402  (the tables' reader and the host traversal)
import test_bounce_class_host as tc  # noqa: E402  (the class tables' reader)
from test_tile_entry_host import camera_rays  # noqa: E402

NONE, FULL = 0x7FFF, 24


def main():
    cfg = scenes.CONFIGS["c2"]
    T = tb.tables("rtiow")  # C2's scene
    P = T.prims.astype(np.float64)
    ground = int(np.argmax(np.abs(P[:, 3])))
    rng = np.random.default_rng(14)
    forms = {f: tc.class_tables("rtiow", f) for f in (1, 2)}
    print(f"tree: {T.info.num_nodes} nodes + {T.info.num_chain_nodes} chain nodes, {len(T.records)} records, grid "
          f"{tuple(T.info.grid_dim)}; form 2 adds {forms[2].info.num_class_nodes} chain nodes; class records "
          f"{len(T.records) * 24}, distinct {len(np.unique(forms[2].records.reshape(-1, 8), axis=0))} (form 2)")
    # the visible ground (pixel centres of a 192 x 108 grid) and the spheres' upper halves
    w, h = 192, 108
    xs, gs = np.meshgrid(np.arange(w), np.arange(h))
    o, d = camera_rays(cfg.inputs(), w, h, xs.ravel(), gs.ravel(), 0.5, 0.5)
    o, d = o.astype(np.float64), d.astype(np.float64)
    t_all = tb.brute_force(T, o, d)
    t_g = tb._prim_t(np.broadcast_to(P[ground], (len(o), 8)), o, d, np.full(len(o), np.inf))
    vis = np.isfinite(t_g) & (t_g == t_all)
    gp = o[vis] + t_g[vis, None] * d[vis]
    gn = (gp - P[ground, 0:3]) / np.abs(P[ground, 3])
    idx = rng.integers(0, len(P) - 1, 4000)
    idx = np.where(idx >= ground, idx + 1, idx)
    v = rng.normal(size=(len(idx), 3))
    v /= np.linalg.norm(v, axis=1)[:, None]
    v[:, 1] = np.abs(v[:, 1])
    sp = P[idx, 0:3] + np.abs(P[idx, 3:4]) * v
    print("origins | chain references per bounce ray: full, form 1, form 2 | host node visits per ray: full, form 1, form 2 | class 24")
    for name, org, nrm in ((f"visible ground ({len(gp)} points)", gp, gn), ("sphere surfaces, upper half", sp, v)):
        q = rng.normal(size=org.shape)
        q *= (rng.uniform(size=(len(org), 1)) ** (1.0 / 3.0)) / np.linalg.norm(q, axis=1)[:, None]
        org32 = org.astype(np.float32).astype(np.float64)
        dir32 = (nrm + q).astype(np.float32).astype(np.float64)
        cls = tc.classes_of("rtiow", org32, dir32)
        rec_idx = T.grid[tc.cells_of(T, org32)]
        refs, visits = [], []
        for label, CT, c in (("full", forms[1], np.full(len(cls), FULL)), ("form 1", forms[1], cls), ("form 2", forms[2], cls)):
            rec = CT.records[rec_idx, c]
            start = [[0] if e[0] == 0 else [int(r) for r in e if r != NONE] for e in rec]
            t, nv = tb.traverse(CT.T, org32, dir32, start)
            if refs:
                assert np.array_equal(t, t_full, equal_nan=True), label
            else:
                t_full = t
            refs.append(np.mean([len(s) - 1 for s in start]))
            visits.append(nv.mean())
        print(f"{name} | {refs[0]:.2f} {refs[1]:.2f} {refs[2]:.2f} | {visits[0]:.2f} {visits[1]:.2f} {visits[2]:.2f} | "
              f"{(cls == FULL).mean() * 100:.1f} %")


if __name__ == "__main__":
    main()
