"""GPU tests of the direction classes of the v3 kernels' bounce entries (render.hip v3_bounce_entry, rt_bounce_entry.h,
rt_set_bounce_classes): a bounce ray's start record lists only the sibling subtrees a ray of its direction class can
reach from its origin's grid cell.  Nothing a frame computes may change: with the switch at 0 (the full records), 1
(existing chain nodes) and 2 (re-paired), pixels, advanced XORWOW states and ray counts are bit-equal to the oracle's —
and so to each other.  There are no tolerances.

Frames: 128x72 (whole tiles) and 67x45 (partial tiles at the right and bottom edges), 8 samples, depth 8, variant 3
forced, on RTIOW, the five-primitive "ends" scene of tests/test_gpu_path_end.py, the touching-rectangles scene (ties and
box faces) and the Cornell box (rectangles only), in XORWOW with both state layouts and in Philox.
"""
from __future__ import annotations

import functools

import numpy as np
import pytest
import torch

from adversarial_scene import ADVERSARIAL_CONFIG, adversarial_scene_tiled
from cudaraytracer_amd import abi, scenes
from cudaraytracer_amd._lib import lib
from cudaraytracer_amd.renderer import DeviceScene, Renderer, set_bounce_classes
from oracle import py_oracle as po
from test_gpu_path_end import _ends_scene

pytestmark = pytest.mark.gpu

SIZES = [(128, 72), (67, 45)]
SPP, DEPTH = 8, 8
FORMS = (0, 1, 2)
MODES = {"xorwow": ("xorwow", "curand"), "xorwow-soa": ("xorwow", "soa"), "philox": ("philox", "curand")}


@pytest.fixture(autouse=True)
def _reset():
    before = lib().rt_set_bounce_classes(0)
    yield
    lib().rt_set_variant(-1)
    lib().rt_set_bounce_entries(1)
    lib().rt_set_bounce_classes(before)


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
def _device_scene(key, form):
    """The scene with the class tables of `form` (a scene carries the form its thread had set when it was created)."""
    set_bounce_classes(form)
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


def _render(key, width, height, mode, form, flags=0, band_rows=8, num_ranks=1, rank=0, entries=1):
    rng, layout = MODES[mode]
    lib().rt_set_variant(3)
    ds = _device_scene(key, form)
    set_bounce_classes(form)
    assert lib().rt_set_bounce_entries(entries) >= 0
    r = Renderer(width, height, band_rows=band_rows, num_ranks=num_ranks, rank=rank, rng=rng, state_layout=layout)
    r.render_init()
    r.counters.zero_()
    r.render(ds, SPP, DEPTH, _SCENES[key][1](), flags=flags, frame=2 if rng == "philox" else None)
    torch.cuda.synchronize()
    assert lib().rt_last_variant() == 3
    return r, r.image().copy(), (r.states()[:, :6].copy() if rng == "xorwow" else None), r.counters.cpu().numpy().copy()


@pytest.mark.parametrize("mode", sorted(MODES))
@pytest.mark.parametrize("key", sorted(_SCENES))
@pytest.mark.parametrize("width, height", SIZES)
def test_frames_are_the_reference_in_every_form(width, height, key, mode):
    philox = mode == "philox"
    ref, st, rays = _oracle(key, width, height, philox)
    for form in FORMS:
        _, img, states, cnt = _render(key, width, height, mode, form)
        bad = np.argwhere(img != ref)
        assert len(bad) == 0, f"bounce classes {form}: {len(bad)} pixels differ, first {bad[:4].tolist()}"
        if not philox:
            np.testing.assert_array_equal(states, st[:, :6], err_msg=f"bounce classes {form}")
        assert int(cnt[0]) == rays, (form, int(cnt[0]), rays)


@pytest.mark.parametrize("form", (1, 2))
def test_two_ranks_of_16_row_bands(form):
    width, height = SIZES[0]
    ref, st, rays = _oracle("rtiow", width, height, False)
    full = np.zeros((height, width), np.uint32)
    states = np.zeros((height * width, 6), np.uint32)
    total = 0
    for rank in range(2):
        r, img, s, cnt = _render("rtiow", width, height, "xorwow", form, band_rows=16, num_ranks=2, rank=rank)
        full[r.rows] = img
        states.reshape(height, width, 6)[r.rows] = s.reshape(len(r.rows), width, 6)
        total += int(cnt[0])
    np.testing.assert_array_equal(full, ref)
    np.testing.assert_array_equal(states, st[:, :6])
    assert total == rays


def test_box_tests_fall_and_the_entries_switch_overrides_the_classes():
    """RT_FLAG_COUNT_TESTS on RTIOW: counters[1] (box tests) is strictly lower with the class records than with the full
    ones; with rt_set_bounce_entries(0) every bounce ray starts at the root whatever the classes say."""
    width, height = SIZES[1]
    ref, _, rays = _oracle("rtiow", width, height, False)
    boxes, root = {}, {}
    for form in FORMS:
        _, img, _, cnt = _render("rtiow", width, height, "xorwow", form, flags=abi.RT_FLAG_COUNT_TESTS)
        np.testing.assert_array_equal(img, ref)
        assert int(cnt[0]) == rays
        boxes[form] = int(cnt[1])
        _, img, _, cnt = _render("rtiow", width, height, "xorwow", form, flags=abi.RT_FLAG_COUNT_TESTS, entries=0)
        np.testing.assert_array_equal(img, ref)
        root[form] = int(cnt[1])
    print(f"box tests: full {boxes[0]}, existing pairs {boxes[1]}, re-paired {boxes[2]}; from the root {root[0]}")
    assert boxes[1] < boxes[0] and boxes[2] < boxes[0]
    assert root[0] == root[1] == root[2] > boxes[0]


def test_a_scene_with_32_bit_references_renders_as_before():
    sc = scenes.sphere_field(9000, 6)
    inputs = scenes.CONFIGS["c2"].inputs()
    width, height = SIZES[1]
    got = []
    for form in (0, 2):
        lib().rt_set_variant(3)
        set_bounce_classes(form)
        ds = DeviceScene(sc)
        r = Renderer(width, height, band_rows=8)
        r.render_init()
        r.counters.zero_()
        r.render(ds, SPP, DEPTH, inputs)
        torch.cuda.synchronize()
        got.append((r.image().copy(), r.states()[:, :6].copy(), int(r.counters[0])))
        ds.close()
    np.testing.assert_array_equal(got[0][0], got[1][0])
    np.testing.assert_array_equal(got[0][1], got[1][1])
    assert got[0][2] == got[1][2] > 0


def test_scenes_have_class_tables():
    """(CPU facts the cases above rest on: RTIOW and the touching scene drop siblings in both forms.)"""
    import ctypes as C
    for key in ("rtiow", "touching"):
        d = _scene(key).desc()
        for form in (1, 2):
            info = abi.BounceClassInfo()
            assert lib().rt_bounce_class_entries_host(C.byref(d), form, 0, None, None, None, None, None, None, 0, None,
                                                      C.byref(info)) == 0
            assert info.form == form and info.num_records > 0
            assert (info.num_class_nodes > 0) == (form == 2)
