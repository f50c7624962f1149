"""GPU tests of the v3 kernels' per-tile entry records (render.hip v3_start_camera_trace, tile_entries_kernel;
csrc/rt_tile_entry.h): camera rays of a whole 8×8 tile start at the leaves the tile's beam can touch instead of the
root.  Nothing a frame computes may change: pixels, advanced RNG states and ray counts are bit-equal to the oracle and
to the same frame with the feature switched off (RT_TUNE_TILE_ENTRIES 0), while the counting build shows fewer box
tests.

Cameras: C2's own (at these sizes a tile's beam is wide: most tiles keep the root, the sky tiles carry one leaf) and the
same view at fov 4 (every whole tile carries 5 to 8 leaves: the record's stack entries are all in use).
"""
from __future__ import annotations

import functools

import numpy as np
import pytest
import torch

from cudaraytracer_amd import abi, scenes
from cudaraytracer_amd._lib import lib
from cudaraytracer_amd.renderer import DeviceScene, Renderer
from oracle import py_oracle as po

pytestmark = pytest.mark.gpu

SPP, DEPTH = 3, 3
SIZES = [(40, 24), (37, 21)]
WIDE_SPHERES = 8191  # + the ground: 8192 primitives, the smallest scene whose references need 32 bits


@pytest.fixture(autouse=True)
def _reset():
    yield
    lib().rt_set_variant(-1)
    lib().rt_set_tuning(abi.RT_TUNE_TILE_ENTRIES, 1)


def _zoom_inputs():
    return scenes.camera_inputs((13.0, 2.0, 3.0), scenes.normalized((-13.0, -1.6, -3.0)), 4.0)


def _moved_rtiow():
    sc = scenes.builtin(scenes.SCENE_RTIOW)
    for h in sc.hittables:
        if h.radius < 0.5:  # the small spheres: 0.3 along x, 0.1 up
            h.center[0] += 0.3
            h.center[1] += 0.1
    return sc


_SCENES = {
    "rtiow": lambda: scenes.builtin(scenes.SCENE_RTIOW),
    "rtiow_moved": _moved_rtiow,
    "wide": lambda: scenes.sphere_field(WIDE_SPHERES, 3),
    "textured": lambda: scenes.builtin(scenes.SCENE_TEXTURED),
}
_CAMERAS = {
    "c2": lambda: scenes.CONFIGS["c2"].inputs(),
    "zoom": _zoom_inputs,
    "c5": lambda: scenes.CONFIGS["c5"].inputs(),
}


@functools.lru_cache(maxsize=None)
def _scene(key):
    return _SCENES[key]()


@functools.lru_cache(maxsize=None)
def _oracle(key, cam, width, height, philox, ltr, frame=0):
    """The reference's frame — pixels, advanced XORWOW states, ray count — rendered once and left unchanged."""
    st = None if philox else po.init_states(width, height)
    ref, _, cnt = po.render(po.OracleScene(_scene(key)), width, height, SPP, DEPTH, _CAMERAS[cam](), st, philox=philox,
                            seed=1984, frame=frame, rius_order=0 if ltr else 1, threads=8)
    ref.setflags(write=False)
    if st is not None:
        st.setflags(write=False)
    return ref, st, int(cnt.rays)


def _render(ds, cam, width, height, variant, rng, entries, ltr=False, frame=0, count=False, band_rows=8):
    lib().rt_set_variant(variant)
    assert lib().rt_set_tuning(abi.RT_TUNE_TILE_ENTRIES, entries) >= 0
    r = Renderer(width, height, band_rows=band_rows, rng=rng)
    r.render_init()
    r.counters.zero_()
    flags = (abi.RT_FLAG_RIUS_LEFT_TO_RIGHT if ltr else 0) | (abi.RT_FLAG_COUNT_TESTS if count else 0)
    r.render(ds, SPP, DEPTH, _CAMERAS[cam](), flags=flags, frame=frame if rng == "philox" else None)
    torch.cuda.synchronize()
    assert lib().rt_last_variant() == variant
    return r.image().copy(), (r.states()[:, :6].copy() if rng == "xorwow" else None), [int(x) for x in r.counters.tolist()]


def _check(key, cam, width, height, variant, rng, ltr=False, frame=0):
    """The frame with the entry records and without: both the oracle's, so equal to each other."""
    philox = rng == "philox"
    ref, st, rays = _oracle(key, cam, width, height, philox, ltr, frame if philox else 0)
    ds = DeviceScene(_scene(key))
    for entries in (1, 0):
        img, states, cnt = _render(ds, cam, width, height, variant, rng, entries, ltr, frame)
        bad = np.argwhere(img != ref)
        assert len(bad) == 0, f"entries {entries}: {len(bad)} pixels differ, first {bad[:4].tolist()}"
        if not philox:
            np.testing.assert_array_equal(states, st[:, :6])
        assert cnt[0] == rays, (entries, cnt[0], rays)


@pytest.mark.parametrize("ltr", [False, True])
@pytest.mark.parametrize("rng", ["xorwow", "philox"])
@pytest.mark.parametrize("variant", [2, 3])
@pytest.mark.parametrize("width, height", SIZES)
def test_rtiow_frames_are_the_reference(width, height, variant, rng, ltr):
    _check("rtiow", "c2", width, height, variant, rng, ltr, frame=2)


@pytest.mark.parametrize("rng", ["xorwow", "philox"])
@pytest.mark.parametrize("variant", [2, 3])
@pytest.mark.parametrize("width, height", SIZES)
def test_zoomed_frames_are_the_reference(width, height, variant, rng):
    """fov 4: the whole tiles carry 5 to 8 leaves each, the ragged frame's partial tiles start at the root."""
    _check("rtiow", "zoom", width, height, variant, rng, frame=1)


@pytest.mark.parametrize("rng", ["xorwow", "philox"])
def test_wide_scene_keeps_the_root(rng):
    """8192 primitives: 32-bit references do not fit the record, the WIDE build of variant 3 starts at the root."""
    _check("wide", "c2", 40, 24, 3, rng)


@pytest.mark.parametrize("variant", [2, 3])
def test_textured_scene(variant):
    _check("textured", "c5", 40, 24, variant, "xorwow")


def test_two_ranks_reassemble_the_frame():
    """Bands of 8 rows over 2 ranks: each rank's records follow its tiles' global rows."""
    width, height = 40, 48
    ref, _, rays = _oracle("rtiow", "zoom", width, height, True, False, 0)
    ds = DeviceScene(_scene("rtiow"))
    lib().rt_set_variant(3)
    full = np.zeros((height, width), np.uint32)
    total = 0
    for rank in range(2):
        r = Renderer(width, height, band_rows=8, num_ranks=2, rank=rank, rng="philox")
        r.render_init()
        r.counters.zero_()
        r.render(ds, SPP, DEPTH, _zoom_inputs(), frame=0)
        torch.cuda.synchronize()
        full[r.rows] = r.image()
        total += int(r.counters[0])
    np.testing.assert_array_equal(full, ref)
    assert total == rays


def test_table_follows_camera_and_scene():
    """One Renderer (one stream, one tile grid: one table): the camera changes between frames, then the scene is edited
    (DeviceScene.edited), then the first camera and scene return — every frame is its own reference, so the table was
    refilled each time."""
    width, height = 40, 24
    lib().rt_set_variant(3)
    r = Renderer(width, height, band_rows=8, rng="philox")
    r.render_init()
    base = DeviceScene(_scene("rtiow"))
    moved = base.edited(_scene("rtiow_moved").hittables)
    for frame, (ds, key, cam) in enumerate([(base, "rtiow", "zoom"), (base, "rtiow", "c2"), (base, "rtiow", "zoom"),
                                            (moved, "rtiow_moved", "zoom"), (base, "rtiow", "zoom")]):
        ref, _, rays = _oracle(key, cam, width, height, True, False, frame)
        r.counters.zero_()
        r.render(ds, SPP, DEPTH, _CAMERAS[cam](), frame=frame)
        torch.cuda.synchronize()
        bad = np.argwhere(r.image() != ref)
        assert len(bad) == 0, f"frame {frame}: {len(bad)} pixels differ, first {bad[:4].tolist()}"
        assert int(r.counters[0]) == rays


def test_box_tests_fall_and_rays_stay():
    """The counting build on the RTIOW frame: the same rays, fewer box tests."""
    ds = DeviceScene(_scene("rtiow"))
    ref, _, rays = _oracle("rtiow", "zoom", 40, 24, False, False)
    img1, _, on = _render(ds, "zoom", 40, 24, 3, "xorwow", 1, count=True)
    img0, _, off = _render(ds, "zoom", 40, 24, 3, "xorwow", 0, count=True)
    np.testing.assert_array_equal(img1, ref)
    np.testing.assert_array_equal(img0, ref)
    print(f"rays {on[0]}, box tests per ray {on[1] / on[0]:.2f} with the records, {off[1] / off[0]:.2f} without; "
          f"primitive tests per ray {on[2] / on[0]:.2f} / {off[2] / off[0]:.2f}")
    assert on[0] == off[0] == rays
    assert on[1] < off[1]


@pytest.mark.parametrize("threshold", [64, 1])
def test_regeneration_threshold(threshold):
    """RT_TUNE_REGEN_THRESHOLD 64 / 1: traversal calls end as soon as one lane finishes / only when all have — a camera
    ray's leaf chain is walked within one call either way."""
    prev = lib().rt_set_tuning(abi.RT_TUNE_REGEN_THRESHOLD, threshold)
    assert prev >= 0
    try:
        _check("rtiow", "zoom", 40, 24, 3, "xorwow")
        _check("rtiow", "zoom", 37, 21, 3, "philox", frame=1)
    finally:
        lib().rt_set_tuning(abi.RT_TUNE_REGEN_THRESHOLD, prev)
