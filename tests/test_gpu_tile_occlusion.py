"""GPU tests of the entry records' occlusion culling (csrc/rt_tile_entry.h tile_occlusion, rt_set_tile_occlusion;
render.hip tile_entries_kernel): the records lose the candidates hidden behind a sphere that covers their tile, and
nothing a frame computes changes — pixels, advanced XORWOW states and ray counts are the oracle's with the switch on
and off, the device pre-pass writes the records rt_tile_entries_host computes, and the counting build shows fewer
primitive tests.

Scenes: tests/occlusion_scene.py's built scene at 64 × 48 (40 of its 48 tiles lose a candidate) and RTIOW under C2's
camera at 192 × 112; 3 samples, depth 3; variant 3 in both RNG modes and variant 2.
"""
from __future__ import annotations

import ctypes as C
import functools

import numpy as np
import pytest
import torch

import occlusion_scene as oc
from cudaraytracer_amd import abi, scenes
from cudaraytracer_amd._lib import lib
from cudaraytracer_amd.renderer import DeviceScene, Renderer
from oracle import py_oracle as po

pytestmark = pytest.mark.gpu

SPP, DEPTH = 3, 3
_SCENES = {
    "built": (lambda: oc.scene("tangent"), lambda: oc.inputs(), oc.WIDTH, oc.HEIGHT),
    "rtiow": (lambda: scenes.builtin(scenes.SCENE_RTIOW), lambda: scenes.CONFIGS["c2"].inputs(), 192, 112),
}
_MODES = [(3, "xorwow"), (3, "philox"), (2, "xorwow")]


@pytest.fixture(autouse=True)
def _reset():
    yield
    lib().rt_set_variant(-1)
    lib().rt_set_tile_occlusion(1)


@functools.lru_cache(maxsize=None)
def _scene(key):
    return _SCENES[key][0]()


@functools.lru_cache(maxsize=None)
def _oracle(key, philox):
    """The reference's frame — pixels, advanced XORWOW states, ray count — rendered once and left unchanged."""
    _, inputs, width, height = _SCENES[key]
    st = None if philox else po.init_states(width, height)
    ref, _, cnt = po.render(po.OracleScene(_scene(key)), width, height, SPP, DEPTH, inputs(), st, philox=philox,
                            seed=1984, frame=1 if philox else 0, threads=8)
    ref.setflags(write=False)
    if st is not None:
        st.setflags(write=False)
    return ref, st, int(cnt.rays)


def _render(ds, key, variant, rng, on, count=False):
    _, inputs, width, height = _SCENES[key]
    lib().rt_set_variant(variant)
    assert lib().rt_set_tile_occlusion(on) >= 0
    r = Renderer(width, height, band_rows=8, rng=rng)
    r.render_init()
    r.counters.zero_()
    r.render(ds, SPP, DEPTH, inputs(), flags=abi.RT_FLAG_COUNT_TESTS if count else 0, frame=1 if rng == "philox" else None)
    torch.cuda.synchronize()
    assert lib().rt_last_variant() == variant
    return r.image().copy(), (r.states()[:, :6].copy() if rng == "xorwow" else None), [int(x) for x in r.counters.tolist()]


@pytest.mark.parametrize("variant, rng", _MODES)
@pytest.mark.parametrize("key", list(_SCENES))
def test_frames_are_the_reference(key, variant, rng):
    """Switch on and off: both the oracle's frame, states and ray count, so equal to each other."""
    ref, st, rays = _oracle(key, rng == "philox")
    ds = DeviceScene(_scene(key))
    for on in (1, 0):
        img, states, cnt = _render(ds, key, variant, rng, on)
        bad = np.argwhere(img != ref)
        assert len(bad) == 0, f"occlusion {on}: {len(bad)} pixels differ, first {bad[:4].tolist()}"
        if st is not None:
            np.testing.assert_array_equal(states, st[:, :6], err_msg=f"occlusion {on}")
        assert cnt[0] == rays, (on, cnt[0], rays)


@pytest.mark.parametrize("on", [1, 0])
@pytest.mark.parametrize("key", list(_SCENES))
def test_device_table_is_the_host_table(key, on):
    """tile_entries_kernel and rt_tile_entries_host run one classifier: the same records, bit for bit."""
    _, inputs, width, height = _SCENES[key]
    sc, inp = _scene(key), inputs()
    ds = DeviceScene(sc)
    t = abi.Tiling(8, 1, 0, height)
    tiles = ((width + 7) // 8) * ((height + 7) // 8)
    assert lib().rt_set_tile_occlusion(on) >= 0
    host = np.zeros((tiles, 4), np.uint32)
    d = sc.desc()
    assert lib().rt_tile_entries_host(C.byref(d), C.byref(inp), width, height, C.byref(t), 0, 0, tiles,
                                      host.ctypes.data_as(C.POINTER(C.c_uint32))) == 0, lib().rt_last_error()
    dev = torch.zeros(tiles * 4, dtype=torch.int32, device="cuda")
    rc = lib().rt_tile_entries_device(ds.handle, C.byref(inp), width, height, C.byref(t), 0, C.c_void_p(dev.data_ptr()),
                                      C.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0, lib().rt_last_error()
    torch.cuda.synchronize()
    got = dev.cpu().numpy().view(np.uint32).reshape(tiles, 4)
    np.testing.assert_array_equal(got, host)
    assert (host[:, 0] & 0xFFFF != 0).any()  # (records with candidates, not "root" throughout)


@pytest.mark.parametrize("key", list(_SCENES))
def test_primitive_tests_fall_and_rays_stay(key):
    """The counting build: the same frame and rays, fewer primitive tests with the switch on."""
    ref, _, rays = _oracle(key, False)
    ds = DeviceScene(_scene(key))
    img1, _, on = _render(ds, key, 3, "xorwow", 1, count=True)
    img0, _, off = _render(ds, key, 3, "xorwow", 0, count=True)
    np.testing.assert_array_equal(img1, ref)
    np.testing.assert_array_equal(img0, ref)
    print(f"{key}: rays {on[0]}, primitive tests per ray {on[2] / on[0]:.3f} with the culling, {off[2] / off[0]:.3f} without")
    assert on[0] == off[0] == rays
    assert on[2] < off[2]


def test_switch_refills_the_table():
    """One Renderer (one stream, one tile grid: one table): the switch changes between frames of the same camera and
    scene, and the counting build's primitive tests follow it — the table was refilled each time."""
    key = "built"
    _, inputs, width, height = _SCENES[key]
    ds = DeviceScene(_scene(key))
    lib().rt_set_variant(3)
    r = Renderer(width, height, band_rows=8, rng="philox")
    r.render_init()
    tests = []
    for on in (1, 0, 1):
        assert lib().rt_set_tile_occlusion(on) >= 0
        r.counters.zero_()
        r.render(ds, SPP, DEPTH, inputs(), flags=abi.RT_FLAG_COUNT_TESTS, frame=1)
        torch.cuda.synchronize()
        np.testing.assert_array_equal(r.image(), _oracle(key, True)[0])
        tests.append(int(r.counters[2]))
    assert tests[0] == tests[2] < tests[1]
