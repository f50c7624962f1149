"""CPU tests of the v3 kernels' per-tile entry records (csrc/rt_tile_entry.h through rt_tile_entries_host, the
classifier the device pre-pass runs): the records are conservative — the primitive every camera ray of a tile hits
lies in one of the tile's candidate leaves — and the cases that must keep the root do.

The closest hit is the oracle's: brute force over the scene's hittables with orc_hittable_hit, strict (0.001, FLT_MAX),
shrinking t_max as it goes (sphere-only scenes: the same test vectorised in numpy with Sphere::Hit's binary32
operations, as tests/test_gpu_v3_visit.py does), on camera rays built with camera_ray's operations (Kernel.cu:139-146)
at the jitters that reach a pixel's corners, (2^-24, 1], and its middle.
"""
from __future__ import annotations

import ctypes as C
import functools

import numpy as np
import pytest

from adversarial_scene import ADVERSARIAL_CONFIG, adversarial_scene_tiled
from cudaraytracer_amd import abi, scenes
from cudaraytracer_amd._lib import lib
from oracle import py_oracle as po

ROOT_MARK, NONE = 0, 0x7FFF
f32 = np.float32
# jitters (xi1, xi2): a pixel's four corners (curand_uniform draws from (0, 1]) and its middle
JITTERS = [(2.0 ** -24, 2.0 ** -24), (1.0, 2.0 ** -24), (2.0 ** -24, 1.0), (1.0, 1.0), (0.5, 0.5)]


def records(sc, inputs, width, height, tiling=None, flags=0):
    """(tiles, 8) entries of every tile of the rank's local rows."""
    t = tiling or abi.Tiling(height, 1, 0, height)
    tiles = ((width + 7) // 8) * ((t.local_rows + 7) // 8)
    out = np.zeros((tiles, 4), np.uint32)
    d = sc.desc()
    rc = lib().rt_tile_entries_host(C.byref(d), C.byref(inputs), width, height, C.byref(t), flags, 0, tiles,
                                    out.ctypes.data_as(C.POINTER(C.c_uint32)))
    assert rc == 0, lib().rt_last_error()
    return np.stack([out & 0xFFFF, out >> 16], axis=2).reshape(tiles, 8)


@functools.lru_cache(maxsize=None)
def _prim_source(key):
    sc = _SCENES[key]()
    d = sc.desc()
    info = abi.HostTablesInfo()
    assert lib().rt_build_host_tables(C.byref(d), None, None, None, None, C.byref(info)) == 0
    src = (C.c_int32 * max(1, info.num_prims))()
    nodes = (C.c_float * (16 * max(1, info.num_nodes)))()
    prims = (C.c_float * (8 * max(1, info.num_prims)))()
    mats = (C.c_float * (12 * max(1, info.num_materials)))()
    assert lib().rt_build_host_tables(C.byref(d), nodes, prims, mats, src, C.byref(info)) == 0
    return np.array(src[: info.num_prims], np.int64), int(info.depth)


def candidates(entries, src):
    """The hittable indices in a record's leaves (a leaf reference is ~(first << 2 | count - 1) in 16 bits)."""
    out = set()
    for e in entries:
        if e == NONE:
            continue
        assert e >= 0x8000, f"entry {e:#x} is not a leaf reference"
        leaf = int(e) ^ 0xFFFF
        first, count = leaf >> 2, (leaf & 3) + 1
        out.update(int(s) for s in src[first:first + count])
    return out


def camera_rays(inputs, width, height, xs, gs, xi1, xi2):
    """camera_ray (render.hip, Kernel.cu:130-146) in binary32 for pixels (xs, gs) at one jitter: origins, directions."""
    up = np.array(list(inputs.up), f32)
    fw = np.array(list(inputs.orientation), f32)
    org = np.array(list(inputs.origin), f32)
    c = np.array([up[1] * fw[2] - up[2] * fw[1], -(up[0] * fw[2] - up[2] * fw[0]), up[0] * fw[1] - up[1] * fw[0]], f32)
    right = (f32(1.0) / np.sqrt((c[0] * c[0] + c[1] * c[1]) + c[2] * c[2], dtype=f32)) * c
    fov = f32(inputs.fov)
    k10 = (f32(1.0) / fov) * f32(10.0)
    w = f32(width)
    u = ((xs.astype(f32) - f32(width) / f32(2.0)) + f32(xi1)) / w
    v = ((f32(height) / f32(2.0) - gs.astype(f32)) + f32(xi2)) / w
    dist = u[:, None] * right[None, :] + v[:, None] * up[None, :]
    start = (f32(inputs.near_plane) * dist + org) + fov * fw
    second = (f32(inputs.far_plane) * dist + k10 * fw) + org
    d = second - start
    n = np.sqrt((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2], dtype=f32)
    return start.astype(f32), (d / n[:, None]).astype(f32)


def closest_hits(sc, o, d):
    """Index of the hittable each ray hits first (-1: none)."""
    hs = [h for h in sc.hittables]
    if all(h.type == abi.RT_SPHERE for h in hs):
        act = np.array([bool(h.is_active) for h in hs])
        c = np.array([list(h.center) for h in hs], f32)
        r2 = np.array([h.radius * h.radius for h in hs], f32)
        best = np.full(len(o), np.inf, f32)
        who = np.full(len(o), -1, np.int64)
        a = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
        for k in np.nonzero(act)[0]:
            oc = o - c[k]
            b = (oc[:, 0] * d[:, 0] + oc[:, 1] * d[:, 1]) + oc[:, 2] * d[:, 2]
            cc = ((oc[:, 0] * oc[:, 0] + oc[:, 1] * oc[:, 1]) + oc[:, 2] * oc[:, 2]) - r2[k]
            disc = b * b - a * cc
            with np.errstate(invalid="ignore"):
                sq = np.sqrt(np.where(disc > 0, disc, f32(1.0)))
                tn, tf = (-b - sq) / a, (-b + sq) / a
            t = np.where(tn > f32(0.001), tn, np.where(tf > f32(0.001), tf, np.inf)).astype(f32)
            t = np.where(disc > 0, t, np.inf)
            closer = t < best
            best, who = np.where(closer, t, best), np.where(closer, k, who)
        return who
    L = po.lib()
    F3 = C.c_float * 3
    who = np.full(len(o), -1, np.int64)
    rec = po.Hit()
    for r in range(len(o)):
        op, dp, tmax = F3(*o[r]), F3(*d[r]), float(np.finfo(f32).max)
        for i, h in enumerate(hs):
            if h.is_active and L.orc_hittable_hit(C.byref(h), op, dp, 0.001, tmax, C.byref(rec)):
                tmax, who[r] = rec.t, i
    return who


def _inside_camera():
    # inside RTIOW's sphere field, a wide view: beams near the eye meet many leaves
    return scenes.camera_inputs((0.5, 0.6, 0.5), scenes.normalized((-1.0, -0.2, -0.4)), 90.0)


_SCENES = {
    "rtiow": lambda: scenes.builtin(scenes.SCENE_RTIOW),
    "default": lambda: scenes.builtin(scenes.SCENE_DEFAULT_WORLD),
    "touching": adversarial_scene_tiled,
}
_CASES = [
    ("rtiow", lambda: scenes.CONFIGS["c2"].inputs(), 40, 24),
    ("rtiow", lambda: scenes.CONFIGS["c2"].inputs(), 37, 21),
    ("rtiow", _inside_camera, 40, 24),
    ("default", lambda: scenes.CONFIGS["default"].inputs(), 40, 24),
    ("touching", lambda: ADVERSARIAL_CONFIG.inputs(), 40, 24),
]


def _check_conservative(key, inputs, width, height, tiling=None):
    sc = _SCENES[key]()
    src, _ = _prim_source(key)
    t = tiling or abi.Tiling(8, 1, 0, height)  # (bands of 8 rows: a frame of any height has whole tiles)
    rec = records(sc, inputs, width, height, t)
    tiles_x = (width + 7) // 8
    ly, x = np.divmod(np.arange(width * t.local_rows), width)
    band, within = np.divmod(ly, t.band_rows)
    g = (band * t.num_ranks + t.rank) * t.band_rows + within
    tile = (ly // 8) * tiles_x + x // 8
    cand = [None if r[0] == ROOT_MARK else candidates(r, src) for r in rec]
    checked = 0
    for xi1, xi2 in JITTERS:
        who = closest_hits(sc, *camera_rays(inputs, width, height, x, g, xi1, xi2))
        for p in range(len(who)):
            c = cand[tile[p]]
            if c is None or who[p] < 0:
                continue
            checked += 1
            assert int(who[p]) in c, f"pixel ({x[p]}, {g[p]}) jitter ({xi1}, {xi2}): hittable {who[p]} not in tile {tile[p]}'s {sorted(c)}"
    return rec, checked


@pytest.mark.parametrize("case", range(len(_CASES)))
def test_every_camera_ray_hits_a_candidate(case):
    """The conservativeness condition, without exceptions: for every pixel of every tile that carries candidates, at
    every jitter tried, the closest hit's primitive is in the tile's candidate set."""
    key, inputs, width, height = _CASES[case]
    rec, checked = _check_conservative(key, inputs(), width, height)
    tiles_x, tiles_y = (width + 7) // 8, (height + 7) // 8
    full = np.array([[8 * bx + 8 <= width and 8 * by + 8 <= height for bx in range(tiles_x)] for by in range(tiles_y)]).ravel()
    # partial tiles keep the root (their lanes outside the image render pixel 0's ray)
    assert (rec[~full, 0] == ROOT_MARK).all()
    if case == 2:  # the camera inside the sphere field: beams that meet more than 8 leaves keep the root
        assert (rec[full, 0] == ROOT_MARK).any()
    else:
        assert (rec[full, 0] != ROOT_MARK).any() and checked > 0
    # entries are packed from the front: nothing follows a pad
    for r in rec[rec[:, 0] != ROOT_MARK]:
        n = int((r != NONE).sum())
        assert (r[:n] != NONE).all() and (r[n:] == NONE).all()


def test_c2_tiles_carry_few_leaves():
    """C2's own frame (1920×1080, RTIOW): nearly every tile gets candidates, and few of them — what the feature rests
    on (the CPU model of tools/beam_model.py: 99.5 % of tiles with at most 8 leaves, 2.8 on average)."""
    cfg = scenes.CONFIGS["c2"]
    rec = records(_SCENES["rtiow"](), cfg.inputs(), cfg.width, cfg.height)
    assert len(rec) == 240 * 135
    rooted = rec[:, 0] == ROOT_MARK
    n = (rec[~rooted] != NONE).sum(axis=1)
    print("tiles keeping the root: %.2f %%; leaves per tile: mean %.2f, max %d" % (100 * rooted.mean(), n.mean(), n.max()))
    assert rooted.mean() < 0.02
    assert n.mean() < 4.0


def test_c2_frame_sampled_tiles_are_conservative():
    """The same condition on C2's own frame, where a tile's beam is 0.15° wide and nearly every tile carries candidates:
    200 tiles drawn at random and the 200 with the most candidates."""
    cfg = scenes.CONFIGS["c2"]
    sc = _SCENES["rtiow"]()
    src, _ = _prim_source("rtiow")
    inputs = cfg.inputs()
    rec = records(sc, inputs, cfg.width, cfg.height)
    tiles_x = cfg.width // 8
    rng = np.random.default_rng(11)
    busy = np.argsort(-(rec != NONE).sum(axis=1) * (rec[:, 0] != ROOT_MARK))[:200]
    picked = np.unique(np.concatenate([rng.choice(len(rec), 200, replace=False), busy]))
    picked = picked[rec[picked, 0] != ROOT_MARK]
    assert len(picked) >= 300
    lane = np.arange(64)
    x = ((picked % tiles_x) * 8)[:, None] + (lane & 7)[None, :]
    g = ((picked // tiles_x) * 8)[:, None] + (lane >> 3)[None, :]
    cand = [candidates(rec[t], src) for t in picked]
    hits = 0
    for xi1, xi2 in JITTERS:
        who = closest_hits(sc, *camera_rays(inputs, cfg.width, cfg.height, x.ravel(), g.ravel(), xi1, xi2)).reshape(-1, 64)
        for k in range(len(picked)):
            for w in who[k]:
                if w >= 0:
                    hits += 1
                    assert int(w) in cand[k], f"tile {picked[k]}: hittable {w} not in {sorted(cand[k])}"
    assert hits > 0.5 * 5 * 64 * len(picked)


def test_root_markers():
    sc = _SCENES["rtiow"]()
    inputs = scenes.CONFIGS["c2"].inputs()
    # far == near: the rays' common point is at infinity
    flat = abi.InputStruct.from_buffer_copy(inputs)
    flat.far_plane = flat.near_plane
    assert (records(sc, flat, 40, 24)[:, 0] == ROOT_MARK).all()
    # a non-finite camera field
    bad = abi.InputStruct.from_buffer_copy(inputs)
    bad.origin[1] = float("nan")
    assert (records(sc, bad, 40, 24)[:, 0] == ROOT_MARK).all()
    bad = abi.InputStruct.from_buffer_copy(inputs)
    bad.fov = float("inf")
    assert (records(sc, bad, 40, 24)[:, 0] == ROOT_MARK).all()
    # band_rows not a multiple of 8: a tile's rows would straddle bands
    assert (records(sc, inputs, 40, 24, abi.Tiling(12, 1, 0, 24))[:, 0] == ROOT_MARK).all()
    # an empty scene has no node to start at
    empty = scenes.Scene((abi.HittableDesc * 0)(), sc.materials, [])
    assert (records(empty, inputs, 40, 24)[:, 0] == ROOT_MARK).all()


def test_band_layout_rank_one():
    """16-row bands over 2 ranks, rank 1 of a 40×64 frame (global rows 16-31, 48-63): the beams follow the tiles' global
    rows — conservative on the rank's own pixels, and equal to the whole frame's records of the same rows."""
    inputs = scenes.CONFIGS["c2"].inputs()
    width, height = 40, 64
    t = abi.Tiling(16, 2, 1, 32)
    rec, checked = _check_conservative("rtiow", inputs, width, height, t)
    assert checked > 0
    whole = records(_SCENES["rtiow"](), inputs, width, height)
    tiles_x = 5
    for by in range(4):  # local tile row by = global tile row (by // 2) * 4 + 2 + by % 2
        gby = (by // 2) * 4 + 2 + by % 2
        np.testing.assert_array_equal(rec[by * tiles_x:(by + 1) * tiles_x], whole[gby * tiles_x:(gby + 1) * tiles_x])


def test_faithful_grid_records():
    """RT_FLAG_FAITHFUL_GRID renders whole 16×16 blocks only: tiles inside the grid carry the records they carry without
    the flag, tiles outside it are not rendered and keep the root."""
    inputs = scenes.CONFIGS["c2"].inputs()
    sc = _SCENES["rtiow"]()
    plain = records(sc, inputs, 40, 24)
    faithful = records(sc, inputs, 40, 24, flags=abi.RT_FLAG_FAITHFUL_GRID)  # grid 32 × 16
    tiles_x = 5
    for t in range(15):
        bx, by = t % tiles_x, t // tiles_x
        if bx < 4 and by < 2:
            np.testing.assert_array_equal(faithful[t], plain[t])
        else:
            assert faithful[t, 0] == ROOT_MARK


def test_shallow_tree_limits_the_entries():
    """A record's entries 2… go on the kernel's stack, which holds as many entries as the tree is deep: a tile of a
    depth-d tree carries at most d + 2 entries."""
    sc = scenes.builtin(scenes.SCENE_THREE_SPHERES)
    d = sc.desc()
    info = abi.HostTablesInfo()
    assert lib().rt_build_host_tables(C.byref(d), None, None, None, None, C.byref(info)) == 0
    rec = records(sc, scenes.CONFIGS["c1"].inputs(), 40, 24)
    assert ((rec != NONE).sum(axis=1) <= info.depth + 2).all()


def test_argument_errors():
    sc = _SCENES["default"]()
    d = sc.desc()
    inputs = scenes.CONFIGS["default"].inputs()
    t = abi.Tiling(24, 1, 0, 24)
    out = (C.c_uint32 * 4)()
    assert lib().rt_tile_entries_host(None, C.byref(inputs), 40, 24, C.byref(t), 0, 0, 1, out) < 0
    assert lib().rt_tile_entries_host(C.byref(d), C.byref(inputs), 40, 24, C.byref(t), 0, 15, 1, out) < 0  # 15 tiles: 0-14
    assert lib().rt_tile_entries_host(C.byref(d), C.byref(inputs), 40, 24, C.byref(t), 0, 14, 1, out) == 0
