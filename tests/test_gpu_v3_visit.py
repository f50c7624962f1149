"""GPU tests of the v3 node loop's two visit loops and of the exactness check's stage 2 (render.hip v3_traverse,
bvh_clear): whole frames bit-exact against the oracle — pixels, advanced RNG states, ray counts — on scenes built to
enter the changed code, which the counting build's counters confirm.

The node loop checks whether its lanes hold one node only until a v3_traverse call's first divergent iteration (the
scalar visits of the call's coherent prefix), then visits without the check; a hit that stage 1 of bvh_clear does not
clear — common near the pole of a large sphere — is decided by AABB::Hit on its own reference box (stage 2) and may go
on to the reference replay.
"""
from __future__ import annotations

import ctypes as C
import functools
import math

import numpy as np
import pytest
import torch

from cudaraytracer_amd import abi, scenes
from cudaraytracer_amd._lib import lib
from cudaraytracer_amd.renderer import DeviceScene, Renderer
from oracle import py_oracle as po

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def _variant_reset():
    yield
    lib().rt_set_variant(-1)


def _materials():
    m = (abi.MaterialDesc * 4)()
    for k, (t, fuzz, col) in enumerate([(abi.RT_LAMBERTIAN, 0.0, (0.5, 0.5, 0.5)), (abi.RT_METAL, 0.1, (0.7, 0.6, 0.5)),
                                        (abi.RT_DIELECTRIC, 0.0, (1.0, 1.0, 1.0)), (abi.RT_LAMBERTIAN, 0.0, (0.4, 0.2, 0.1))]):
        m[k].type, m[k].fuzz, m[k].ir = t, fuzz, 1.5
        m[k].albedo.type, m[k].albedo.image = abi.RT_CONSTANT, -1
        m[k].albedo.color[:] = list(col)
    return m


def pole_scene() -> scenes.Scene:
    """RTIOW's ground sphere (radius 1000, pole at the origin) and three unit spheres resting on it around the pole."""
    h = (abi.HittableDesc * 4)()
    h[0].type, h[0].is_active, h[0].material, h[0].radius = abi.RT_SPHERE, 1, 0, 1000.0
    h[0].center[:] = [0.0, -1000.0, 0.0]
    for i, (x, z) in enumerate([(0.0, -3.2), (-2.4, -1.6), (2.4, -1.6)]):
        y = float(np.float32(math.sqrt(1001.0 ** 2 - x * x - z * z) - 1000.0))  # tangent to the ground
        h[i + 1].type, h[i + 1].is_active, h[i + 1].material, h[i + 1].radius = abi.RT_SPHERE, 1, i + 1, 1.0
        h[i + 1].center[:] = [x, y, z]
    return scenes.Scene(h, _materials(), [])


# 2 units above the pole, looking down at POLE_PITCH degrees: the ground within ~2 units of the pole, where a hit's
# |q.y| is within r * 2^-19 of r and stage 1 of bvh_clear cannot clear it, fills the lower part of the frame
POLE_PITCH, POLE_FOV = 35.0, 60.0
POLE = scenes.Config("pole", scenes.SCENE_THREE_SPHERES, 64, 48, 8, 8, (0.0, 2.0, 0.0),
                     scenes.normalized((0.0, -math.sin(math.radians(POLE_PITCH)), -math.cos(math.radians(POLE_PITCH)))),
                     POLE_FOV)


@functools.lru_cache(maxsize=None)
def _oracle(key: str, width: int, height: int, spp: int, depth: int, philox: bool, frame: int = 0):
    """The reference's frame of a named (scene, camera): pixels, advanced XORWOW states, ray count — rendered once."""
    sc, cfg = _SCENES[key]()
    st = None if philox else po.init_states(width, height)
    ref, _, cnt = po.render(po.OracleScene(sc), width, height, spp, depth, cfg.inputs(), st, philox=philox, seed=1984,
                            frame=frame)
    ref.setflags(write=False)
    if st is not None:
        st.setflags(write=False)
    return ref, st, int(cnt.rays)


_SCENES = {
    "pole": lambda: (pole_scene(), POLE),
    "rtiow": lambda: (scenes.builtin(scenes.SCENE_RTIOW), scenes.CONFIGS["c2"]),
    "three": lambda: (scenes.builtin(scenes.SCENE_THREE_SPHERES), scenes.CONFIGS["c1"]),
}


def _check_frame(key, width, height, spp, depth, variant, rng, count=False):
    sc, cfg = _SCENES[key]()
    philox = rng == "philox"
    ref, st, rays = _oracle(key, width, height, spp, depth, philox, 3 if philox else 0)
    lib().rt_set_variant(variant)
    r = Renderer(width, height, rng=rng)
    r.render_init()
    r.counters.zero_()
    r.render(DeviceScene(sc), spp, depth, cfg.inputs(), flags=abi.RT_FLAG_COUNT_TESTS if count else 0,
             frame=3 if philox else None)
    torch.cuda.synchronize()
    assert lib().rt_last_variant() == variant
    img = r.image()
    bad = np.argwhere(img != ref)
    assert len(bad) == 0, f"{len(bad)} pixels differ, first {bad[:4].tolist()}"
    if not philox:
        np.testing.assert_array_equal(r.states()[:, :6], st[:, :6])
    assert int(r.counters[0]) == rays
    return [int(x) for x in r.counters.tolist()]


@pytest.mark.parametrize("rng", ["xorwow", "philox"])
@pytest.mark.parametrize("variant", [2, 3, 4])
def test_pole_frame_is_the_reference(variant, rng):
    """The pole case: stage 2 of the exactness check decides a large share of the shaded hits, and some of them go on
    to the reference replay."""
    _check_frame("pole", POLE.width, POLE.height, POLE.spp, POLE.depth, variant, rng)


@pytest.mark.parametrize("rng", ["xorwow", "philox"])
def test_pole_frame_enters_stage_two_and_the_replay(rng):
    """The same frame through the counting build (variant 3; bit-exact too): the rays that enter stage 2 are at least
    5 % of the frame's rays — a fortiori of its shaded hits, which are rays that hit — and stage 2 sends some of them to
    the replay, so the pole case cannot pass without running the changed code."""
    c = _check_frame("pole", POLE.width, POLE.height, POLE.spp, POLE.depth, 3, rng, count=True)
    rays, replays = c[0], c[17]
    s2_enter, s2_fail, s2_pass = c[23] & 0xffffffff, c[18] >> 32, c[23] >> 32
    print(f"rays {rays}, stage-2 entries {s2_enter}, failures {s2_fail}, replays {replays}, passes with one {s2_pass}")
    assert s2_enter >= 0.05 * rays
    assert s2_fail > 0 and replays >= s2_fail
    assert 0 < s2_pass <= c[6]


@pytest.mark.parametrize("variant", [3, 4])
@pytest.mark.parametrize("key, spp", [("rtiow", 4), ("three", 64)])
@pytest.mark.parametrize("width, height", [(40, 24), (37, 21)])
def test_coherence_transitions_on_small_frames(width, height, key, spp, variant):
    """RTIOW at 4 spp (waves diverge at their first visits) and the 3-sphere scene at 64 spp (whole waves stay on one
    node for many visits, then split) against the oracle, at 40×24 (whole 8×8 tiles, partial 16×16 ones) and at 37×21
    (a ragged last tile in both directions: lanes outside the image stay in their wave as finished lanes)."""
    _check_frame(key, width, height, spp, 8, variant, "xorwow")


@pytest.mark.parametrize("threshold", [64, 1])
@pytest.mark.parametrize("variant", [3, 4])
def test_coherent_prefix_is_per_call(variant, threshold):
    """RT_TUNE_REGEN_THRESHOLD 64 / 1: traversal calls end as soon as one lane finishes / only when all have, and are
    re-entered with lanes at unrelated nodes — the coherent-prefix state must start anew per call."""
    prev = lib().rt_set_tuning(abi.RT_TUNE_REGEN_THRESHOLD, threshold)
    assert prev >= 0
    try:
        _check_frame("three", 40, 24, 64, 8, variant, "xorwow")
        _check_frame("rtiow", 40, 24, 4, 8, variant, "xorwow")
    finally:
        lib().rt_set_tuning(abi.RT_TUNE_REGEN_THRESHOLD, prev)


def _brute_force(sc, o, d):
    """Closest sphere hit per ray with Sphere::Hit's binary32 operations (as test_trace_rays_matches_brute_force_closest_hit)."""
    c = np.array([list(h.center) for h in sc.hittables], np.float32)
    r2 = np.array([h.radius * h.radius for h in sc.hittables], np.float32)
    f = np.float32
    best = np.full(len(o), np.inf, np.float32)
    a = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
    for k in range(len(c)):
        oc = o - c[k]
        b = (oc[:, 0] * d[:, 0] + oc[:, 1] * d[:, 1]) + oc[:, 2] * d[:, 2]
        cc = ((oc[:, 0] * oc[:, 0] + oc[:, 1] * oc[:, 1]) + oc[:, 2] * oc[:, 2]) - r2[k]
        disc = b * b - a * cc
        with np.errstate(invalid="ignore"):
            sq = np.sqrt(np.where(disc > 0, disc, f(1.0)))
            tn, tf = (-b - sq) / a, (-b + sq) / a
        t = np.where(tn > f(0.001), tn, np.where(tf > f(0.001), tf, np.inf)).astype(np.float32)
        best = np.minimum(best, np.where(disc > 0, t, np.inf))
    return best


def _trace(ds, o, d):
    n = len(o)
    rays = np.zeros((2 * n, 4), np.float32)
    rays[0::2, :3], rays[1::2, :3] = o, d
    dr = torch.from_numpy(rays).cuda()
    hits = torch.empty(2 * n, dtype=torch.int32, device="cuda")
    cnt = torch.zeros(abi.COUNTERS_WORDS, dtype=torch.int64, device="cuda")
    assert lib().rt_trace_rays(ds.handle, C.c_void_p(dr.data_ptr()), n, C.c_void_p(hits.data_ptr()),
                               C.c_void_p(cnt.data_ptr()), 1, None) == 0
    torch.cuda.synchronize()
    h = hits.cpu().numpy().reshape(n, 2)
    assert int(cnt[0]) == n
    return np.where(h[:, 0] >= 0, h[:, 1].view(np.float32), np.inf).astype(np.float32), [int(x) for x in cnt.tolist()]


def test_trace_rays_uniform_waves_and_shuffled_rays():
    """rt_trace_rays on 4 096 rays of which every wave's 64 lanes carry the same ray — every node iteration is
    uniform, with all 64 lanes down to the last — and on 4 096 different rays in shuffled order — waves diverge at
    their first visits: both equal the numpy brute force bit for bit."""
    sc = scenes.builtin(scenes.SCENE_RTIOW)
    ds = DeviceScene(sc)
    rng = np.random.default_rng(7)
    n = 4096
    o = np.stack([rng.uniform(-12, 12, n), rng.uniform(0.05, 3.0, n), rng.uniform(-12, 12, n)], 1).astype(np.float32)
    d = rng.normal(size=(n, 3)).astype(np.float32)
    d[: n // 2, 1] = -np.abs(d[: n // 2, 1])
    want = _brute_force(sc, o, d)
    assert np.isfinite(want).mean() > 0.3
    same = np.repeat(np.arange(n // 64), 64)  # wave w: 64 copies of ray w
    got, cnt = _trace(ds, o[same], d[same])
    np.testing.assert_array_equal(got.view(np.uint32), want[same].view(np.uint32))
    assert cnt[11] == cnt[4] > 0  # (the counting build: every node iteration uniform)
    perm = rng.permutation(n)
    got, cnt = _trace(ds, o[perm], d[perm])
    np.testing.assert_array_equal(got.view(np.uint32), want[perm].view(np.uint32))
    assert 0 < cnt[11] < cnt[4]
