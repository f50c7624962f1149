"""GPU tests of the v3 kernels' bounce entries (render.hip v3_bounce_entry, rt_set_bounce_entries): a bounce ray starts
at a BVH leaf near its origin, with the chain of sibling subtrees on its stack, instead of at the root.  Nothing a
frame computes may change: with the switch on and off, pixels, advanced XORWOW states and ray counts are bit-equal to
the oracle's — and so to each other — and the kernel that runs is the same one.  There are no tolerances.

Frames: 40x24 (whole tiles) and 37x21 (partial tiles at the right and bottom edges), 8 samples, depth 8, variant 3
forced (and variant 2 once per RNG), on the five-primitive "ends" scene of tests/test_gpu_path_end.py (every kind of
path end), RTIOW (488 spheres, the ground sphere spanning the grid), the touching-rectangles scene (ties and box faces:
the reference replay runs beside the new start) and the Cornell box (rectangles only), with XORWOW and Philox streams.
"""
from __future__ import annotations

import functools

import numpy as np
import pytest
import torch

from adversarial_scene import ADVERSARIAL_CONFIG, adversarial_scene_tiled
from cudaraytracer_amd import abi, scenes
from cudaraytracer_amd._lib import lib
from cudaraytracer_amd.renderer import DeviceScene, Renderer
from oracle import py_oracle as po
from test_gpu_path_end import _ends_scene

pytestmark = pytest.mark.gpu

SIZES = [(40, 24), (37, 21)]
SPP, DEPTH = 8, 8


@pytest.fixture(autouse=True)
def _reset():
    yield
    lib().rt_set_variant(-1)
    lib().rt_set_bounce_entries(1)
    lib().rt_set_tuning(abi.RT_TUNE_CAMERA_RESOLVE, 1)
    lib().rt_set_tuning(abi.RT_TUNE_PATH_END_STEP, 1)


_SCENES = {
    "ends": (_ends_scene, lambda: scenes.CONFIGS["c2"].inputs()),
    "rtiow": (lambda: scenes.builtin(scenes.SCENE_RTIOW), lambda: scenes.CONFIGS["c2"].inputs()),
    "touching": (adversarial_scene_tiled, lambda: ADVERSARIAL_CONFIG.inputs()),
    "cornell": (lambda: scenes.builtin(scenes.SCENE_CORNELL), lambda: scenes.CONFIGS["c3"].inputs()),
}


@functools.lru_cache(maxsize=None)
def _scene(key):
    return _SCENES[key][0]()


@functools.lru_cache(maxsize=None)
def _device_scene(key):
    return DeviceScene(_scene(key))


@functools.lru_cache(maxsize=None)
def _oracle(key, width, height, philox):
    """The reference's frame — pixels, advanced XORWOW states, ray count — rendered once and left unchanged."""
    st = None if philox else po.init_states(width, height)
    ref, _, cnt = po.render(po.OracleScene(_scene(key)), width, height, SPP, DEPTH, _SCENES[key][1](), st, philox=philox,
                            seed=1984, frame=2 if philox else 0, threads=8)
    ref.setflags(write=False)
    if st is not None:
        st.setflags(write=False)
    return ref, st, int(cnt.rays)


def _render(key, width, height, variant, rng, on):
    lib().rt_set_variant(variant)
    assert lib().rt_set_bounce_entries(on) >= 0
    r = Renderer(width, height, band_rows=8, rng=rng)
    r.render_init()
    r.counters.zero_()
    r.render(_device_scene(key), SPP, DEPTH, _SCENES[key][1](), frame=2 if rng == "philox" else None)
    torch.cuda.synchronize()
    return (r.image().copy(), (r.states()[:, :6].copy() if rng == "xorwow" else None), int(r.counters[0]),
            lib().rt_last_variant())


def _check(key, width, height, variant, rng):
    philox = rng == "philox"
    ref, st, rays = _oracle(key, width, height, philox)
    ran = []
    for on in (1, 0):
        img, states, n, v = _render(key, width, height, variant, rng, on)
        bad = np.argwhere(img != ref)
        assert len(bad) == 0, f"bounce entries {on}: {len(bad)} pixels differ, first {bad[:4].tolist()}"
        if not philox:
            np.testing.assert_array_equal(states, st[:, :6], err_msg=f"bounce entries {on}")
        assert n == rays, (on, n, rays)
        ran.append(v)
    assert ran[0] == ran[1] == variant


@pytest.mark.parametrize("rng", ["xorwow", "philox"])
@pytest.mark.parametrize("key", sorted(_SCENES))
@pytest.mark.parametrize("width, height", SIZES)
def test_frames_are_the_reference_on_and_off(width, height, key, rng):
    _check(key, width, height, 3, rng)


@pytest.mark.parametrize("rng", ["xorwow", "philox"])
def test_uncompacted_v3(rng):
    _check("rtiow", 37, 21, 2, rng)


@pytest.mark.parametrize("knob", [abi.RT_TUNE_CAMERA_RESOLVE, abi.RT_TUNE_PATH_END_STEP])
def test_with_the_other_switches_off(knob):
    assert lib().rt_set_tuning(knob, 0) >= 0
    _check("rtiow", 40, 24, 3, "xorwow")


def test_scenes_have_the_table():
    """(CPU facts the cases above rest on: every scene here gets a table, so the switch changes the start.)"""
    import ctypes as C
    for key in _SCENES:
        d = _scene(key).desc()
        info = abi.BounceEntriesInfo()
        assert lib().rt_bounce_entries_host(C.byref(d), None, None, None, None, None, C.byref(info)) == 0
        assert info.num_records > 0, key
