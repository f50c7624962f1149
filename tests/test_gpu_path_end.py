"""GPU tests of the pending path end of the v3 kernels (render.hip MODE_ENDED, RT_TUNE_PATH_END_STEP): in a wave whose
tile's entry record the shading pass's pre-step scans, a path that shade() or the depth limit ends parks its
contribution and waits for the next pass's pre-step, which adds it and resolves the next camera ray by the scan; the
pixel's first camera ray takes the same route.  Nothing a frame computes may change: with the key 1 and 0, pixels,
advanced XORWOW states and ray counts are bit-equal to the oracle's, so there are no tolerances.

The "ends" scene (built here): RTIOW's ground sphere and four unit spheres — Lambertian, Metal with fuzz 1.0, Dielectric
and a DiffuseLight — under C2's camera.  It has no rectangle, so the pre-step is active for every miss, and only five
primitives, so every whole tile's record is scanned (at most 8 primitives).  The kinds of end it holds:
  * the depth limit: the oracle traces fewer rays at depth 3 than at depth 4 (asserted by the fixture);
  * an emitter: with a black background some pixels are lit (asserted by the fixture);
  * an absorbed Metal scatter: by construction — with fuzz 1.0 the scattered direction is reflect + a point of the unit
    ball, which falls below the surface for a large share of the draws (Material.cuh's Metal::Scatter returns false);
  * a camera ray that missed: the sky above the horizon.
Sizes: 40x24 (whole tiles) and 37x21 (the partial tiles at the right and bottom edges keep the root and with it the
parent's route, beside waves on the new one).
"""
from __future__ import annotations

import ctypes as C
import functools

import numpy as np
import pytest
import torch

from cudaraytracer_amd import abi, scenes
from cudaraytracer_amd._lib import lib
from cudaraytracer_amd.renderer import DeviceScene, Renderer
from oracle import py_oracle as po

pytestmark = pytest.mark.gpu

SIZES = [(40, 24), (37, 21)]
KEY = abi.RT_TUNE_PATH_END_STEP


@pytest.fixture(autouse=True)
def _reset():
    yield
    lib().rt_set_variant(-1)
    lib().rt_set_tuning(KEY, 1)
    lib().rt_set_tuning(abi.RT_TUNE_CAMERA_RESOLVE, 1)


def _ends_scene():
    mats = [(abi.RT_LAMBERTIAN, (0.5, 0.5, 0.5), 0.0, 0), (abi.RT_LAMBERTIAN, (0.4, 0.2, 0.1), 0.0, 0),
            (abi.RT_METAL, (0.7, 0.6, 0.5), 1.0, 0), (abi.RT_DIELECTRIC, (1.0, 1.0, 1.0), 0.0, 0),
            (abi.RT_DIFFUSELIGHT, (1.0, 0.9, 0.8), 0.0, 4)]
    m = (abi.MaterialDesc * len(mats))()
    for k, (t, col, fuzz, light) in enumerate(mats):
        m[k].type, m[k].fuzz, m[k].ir, m[k].light_intensity = t, fuzz, 1.5, light
        m[k].albedo.type, m[k].albedo.image = abi.RT_CONSTANT, -1
        m[k].albedo.color[:] = col
    spheres = [((0.0, -1000.0, 0.0), 1000.0, 0), ((-4.0, 1.0, 0.0), 1.0, 1), ((4.0, 1.0, 0.0), 1.0, 2),
               ((0.0, 1.0, 0.0), 1.0, 3), ((2.0, 1.0, 2.5), 1.0, 4)]
    h = (abi.HittableDesc * len(spheres))()
    for k, (c, r, mat) in enumerate(spheres):
        h[k].type, h[k].is_active, h[k].radius, h[k].material = abi.RT_SPHERE, 1, r, mat
        h[k].center[:] = c
    return scenes.Scene(h, m, [])


_C2 = scenes.CONFIGS["c2"]
_SCENES = {
    "ends": _ends_scene,
    "rtiow": lambda: scenes.builtin(scenes.SCENE_RTIOW),
    "cornell": lambda: scenes.builtin(scenes.SCENE_CORNELL),
}
_CAMERAS = {
    "c2": lambda: _C2.inputs(),
    "c2_black": lambda: scenes.camera_inputs(_C2.position, _C2.orientation, _C2.fov, bg_start=(0.0, 0.0, 0.0),
                                             bg_end=(0.0, 0.0, 0.0)),
    "zoom": lambda: scenes.camera_inputs((13.0, 2.0, 3.0), scenes.normalized((-13.0, -1.6, -3.0)), 4.0),
    "c3": lambda: scenes.CONFIGS["c3"].inputs(),  # looks exactly along +z
    "along_x": lambda: scenes.camera_inputs((-800.0, 278.0, 278.0), (1.0, 0.0, 0.0), 40.0),
}


@functools.lru_cache(maxsize=None)
def _scene(key):
    return _SCENES[key]()


@functools.lru_cache(maxsize=None)
def _device_scene(key):
    return DeviceScene(_scene(key))


@functools.lru_cache(maxsize=None)
def _oracle(key, cam, width, height, philox, ltr, frame, spp, depth):
    """The reference's frame — pixels, advanced XORWOW states, ray count — rendered once and left unchanged."""
    st = None if philox else po.init_states(width, height)
    ref, _, cnt = po.render(po.OracleScene(_scene(key)), width, height, spp, depth, _CAMERAS[cam](), st, philox=philox,
                            seed=1984, frame=frame, rius_order=0 if ltr else 1, threads=8)
    ref.setflags(write=False)
    if st is not None:
        st.setflags(write=False)
    return ref, st, int(cnt.rays)


@functools.lru_cache(maxsize=None)
def _ends_scene_checked():
    """The ends scene does what the module's docstring claims (CPU: the oracle and the host classifier alone)."""
    # the depth limit ends paths
    assert _oracle("ends", "c2", 40, 24, False, False, 0, 4, 3)[2] < _oracle("ends", "c2", 40, 24, False, False, 0, 4, 4)[2]
    # emitter ends: nothing but the light sphere lights a pixel under a black sky
    lit = _oracle("ends", "c2_black", 40, 24, False, False, 0, 4, 8)[0]
    assert np.count_nonzero(lit & 0xFFFFFF) > 0
    # every whole tile's record is one the pre-step scans: not "root", at most 8 primitives
    for width, height in SIZES:
        t = abi.Tiling(8, 1, 0, height)
        tx, ty = (width + 7) // 8, (height + 7) // 8
        out = np.zeros((tx * ty, 4), np.uint32)
        d, inputs = _scene("ends").desc(), _CAMERAS["c2"]()
        rc = lib().rt_tile_entries_host(C.byref(d), C.byref(inputs), width, height, C.byref(t), 0, 0, tx * ty,
                                        out.ctypes.data_as(C.POINTER(C.c_uint32)))
        assert rc == 0, lib().rt_last_error()
        e = np.stack([out & 0xFFFF, out >> 16], axis=2).reshape(ty, tx, 8)
        whole = e[: height // 8, : width // 8]
        assert whole.size > 0 and np.all(whole[..., 0] != 0)
        prims = np.where(whole != 0x7FFF, ((whole ^ 0xFFFF) & 3) + 1, 0).sum(axis=2)
        assert prims.max() <= 8 and prims.max() > 0
        if width % 8 or height % 8:  # the partial tiles keep the root
            assert np.all(e[:, width // 8:, 0] == 0) and np.all(e[height // 8:, :, 0] == 0)
    return True


def _render(key, cam, width, height, variant, rng, end_step, ltr=False, frame=0, count=False, spp=3, depth=3):
    lib().rt_set_variant(variant)
    assert lib().rt_set_tuning(KEY, end_step) >= 0
    r = Renderer(width, height, band_rows=8, rng=rng)
    r.render_init()
    r.counters.zero_()
    flags = (abi.RT_FLAG_RIUS_LEFT_TO_RIGHT if ltr else 0) | (abi.RT_FLAG_COUNT_TESTS if count else 0)
    r.render(_device_scene(key), spp, depth, _CAMERAS[cam](), flags=flags, frame=frame if rng == "philox" else None)
    torch.cuda.synchronize()
    assert lib().rt_last_variant() == variant
    return r.image().copy(), (r.states()[:, :6].copy() if rng == "xorwow" else None), [int(x) for x in r.counters.tolist()]


def _check(key, cam, width, height, variant, rng, ltr=False, frame=0, spp=3, depth=3):
    """The frame with the pending end and without: both the oracle's, so equal to each other."""
    philox = rng == "philox"
    ref, st, rays = _oracle(key, cam, width, height, philox, ltr, frame if philox else 0, spp, depth)
    for value in (1, 0):
        img, states, cnt = _render(key, cam, width, height, variant, rng, value, ltr, frame, spp=spp, depth=depth)
        bad = np.argwhere(img != ref)
        assert len(bad) == 0, f"end step {value}: {len(bad)} pixels differ, first {bad[:4].tolist()}"
        if not philox:
            np.testing.assert_array_equal(states, st[:, :6], err_msg=f"end step {value}")
        assert cnt[0] == rays, (value, cnt[0], rays)


@pytest.mark.parametrize("ltr", [False, True])
@pytest.mark.parametrize("variant, rng", [(2, "xorwow"), (3, "xorwow"), (2, "philox")])
@pytest.mark.parametrize("width, height", SIZES)
def test_ends_scene_frames_are_the_reference(width, height, variant, rng, ltr):
    """Depths 1, 2, 3 and 8; 1 sample (only the first-ray route) and 4."""
    assert _ends_scene_checked()
    for depth in (1, 2, 3, 8):
        for spp in (1, 4):
            _check("ends", "c2", width, height, variant, rng, ltr, frame=2, spp=spp, depth=depth)


def test_ends_scene_black_sky():
    """The emitter ends alone light this frame."""
    assert _ends_scene_checked()
    _check("ends", "c2_black", 40, 24, 3, "xorwow", spp=4, depth=8)


@pytest.mark.parametrize("cap", [2, 6, 32])
def test_primitive_cap(cap):
    """RTIOW at fov 4, 5 to 8 references per tile: with the cap 2 every tile keeps the leaf chain and the parent's
    route, with 6 some do — over-cap waves and scanned waves in one frame — and with 32 every record is scanned."""
    assert lib().rt_set_tuning(abi.RT_TUNE_CAMERA_RESOLVE, cap) >= 0
    _check("rtiow", "zoom", 40, 24, 3, "xorwow", spp=3, depth=3)


@pytest.mark.parametrize("cam", ["c3", "along_x"])
@pytest.mark.parametrize("width, height", SIZES)
def test_rectangle_scene(width, height, cam):
    """The Cornell box forced to variant 3: an axis-aligned miss goes to the reference replay, not to the pre-step,
    and the light rectangle ends paths as an emitter.  Both cameras look exactly along an axis."""
    _check("cornell", cam, width, height, 3, "xorwow")


@pytest.mark.parametrize("threshold", [64, 1])
def test_regeneration_threshold(threshold):
    """RT_TUNE_REGEN_THRESHOLD 64 / 1: a shading pass follows as soon as one lane finishes / only when all have — then
    a pass can leave a wave whose only live lanes are pending."""
    assert _ends_scene_checked()
    prev = lib().rt_set_tuning(abi.RT_TUNE_REGEN_THRESHOLD, threshold)
    assert prev >= 0
    try:
        _check("ends", "c2", 40, 24, 3, "xorwow", spp=4, depth=8)
        _check("rtiow", "zoom", 37, 21, 3, "xorwow")
    finally:
        lib().rt_set_tuning(abi.RT_TUNE_REGEN_THRESHOLD, prev)


@pytest.mark.parametrize("spp, depth", [(0, 3), (3, 0)])
def test_no_samples_and_no_depth(spp, depth):
    assert _ends_scene_checked()
    _check("ends", "c2", 40, 24, 3, "xorwow", spp=spp, depth=depth)
    _check("rtiow", "zoom", 37, 21, 3, "xorwow", spp=spp, depth=depth)


def test_two_ranks_reassemble_the_frame():
    """Bands of 8 rows over 2 ranks: each rank's records, and so its waves' routes, follow its tiles' global rows."""
    width, height = 40, 48
    ref, st, rays = _oracle("rtiow", "zoom", width, height, False, False, 0, 3, 3)
    lib().rt_set_variant(3)
    for value in (1, 0):
        assert lib().rt_set_tuning(KEY, value) >= 0
        full = np.zeros((height, width), np.uint32)
        total = 0
        for rank in range(2):
            r = Renderer(width, height, band_rows=8, num_ranks=2, rank=rank, rng="xorwow")
            r.render_init()
            r.counters.zero_()
            r.render(_device_scene("rtiow"), 3, 3, _CAMERAS["zoom"]())
            torch.cuda.synchronize()
            full[r.rows] = r.image()
            total += int(r.counters[0])
        np.testing.assert_array_equal(full, ref, err_msg=f"end step {value}")
        assert total == rays


def test_counting_build_shows_the_route():
    """The counting build at 40x24 on `zoom` (every record scanned at the default cap): the rays are the oracle's with
    the key 1 and 0, and with 1 there are no more shade() passes (word 6) and no more leaf iterations (word 5) than
    with 0 — no camera ray walks a leaf chain any more, and a camera hit is shaded a pass earlier."""
    ref, _, rays = _oracle("rtiow", "zoom", 40, 24, False, False, 0, 3, 3)
    out = {}
    for value in (1, 0):
        img, _, cnt = _render("rtiow", "zoom", 40, 24, 3, "xorwow", value, count=True)
        np.testing.assert_array_equal(img, ref)
        out[value] = cnt
        print(f"end step {value}: rays {cnt[0]}, leaf iterations per 64 rays {64 * cnt[5] / cnt[0]:.2f}, "
              f"shading passes per 64 rays {64 * cnt[6] / cnt[0]:.3f}")
    assert out[1][0] == out[0][0] == rays
    assert out[1][6] <= out[0][6]
    assert out[1][5] <= out[0][5]


def test_switch():
    L = lib()
    assert L.rt_set_tuning(KEY, 0) == 1
    assert L.rt_set_tuning(KEY, 1) == 0
    for bad in (-1, 2, 1 << 20):
        assert L.rt_set_tuning(KEY, bad) < 0
        assert b"path end step" in L.rt_last_error()
    assert L.rt_set_tuning(KEY, 1) == 1  # (a refused value changes nothing)
