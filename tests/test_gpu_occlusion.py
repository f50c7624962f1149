"""rt_occluded_rays on the GPU: any-hit visibility queries with a range per ray.

Scenes and cameras are those of tests/test_gpu_query.py (RTIOW with 16-bit BVH references, sphere_field(9000, 6) with
32-bit ones; 40x24 and 37x21 frames under two 20-degree cameras).  Every call goes to the C entry point directly, with
both outputs filled with 0x5a and 16 guard elements before and after each, checked after the call.  What is compared
bit for bit: the answer over (0.001, FLT_MAX) with rt_trace_rays' closest hit, and the outputs across schedules
(rays_per_lane, the regeneration threshold, repeated calls, batch sizes, output subsets).  What is compared with the
numpy + oracle reference (tests/test_occlusion_host.py): the shadow rays of four frames on decidable rays, and
hand-made ranges on one-primitive scenes, whose expected values are exact."""
from __future__ import annotations

import ctypes as C

import numpy as np
import pytest
import torch

from cudaraytracer_amd import abi, scenes
from cudaraytracer_amd._lib import lib
from cudaraytracer_amd.renderer import DeviceScene

from test_denoise_host import FLT_MAX, UNDECIDABLE_CAP
from test_gpu_query import FRAMES, device_scene, prim_source
from test_occlusion_host import (SHADOW_FRAMES, hand_rays, hittable_hits, occlusion_reference, one_primitive_scene,
                                 shadow_case)
from test_query_host import query_case, query_scene

pytestmark = pytest.mark.gpu

F = np.float32
GUARD = 16   # guard elements before and after every output
FILL = 0x5a  # byte the outputs and their guards are filled with
WIDTH = {"occluded": 1, "blocker": 4}  # bytes per element


def occluded(ds: DeviceScene, rays: torch.Tensor, n: int, outputs=("occluded", "blocker"), rays_per_lane: int = 0,
             count_tests: int | None = None) -> dict:
    """One direct rt_occluded_rays call on the first n rays: {name: numpy array of n elements} (occluded as uint8), after
    checking that the GUARD elements before and after every output kept their fill.  count_tests 0 / 1: with a counter
    buffer, returned as "counters"."""
    bufs, a = {}, abi.OcclusionArgs()
    a.rays = rays.data_ptr()
    for name in outputs:
        bufs[name] = torch.full(((n + 2 * GUARD) * WIDTH[name],), FILL, dtype=torch.uint8, device="cuda")
        setattr(a, name, bufs[name].data_ptr() + GUARD * WIDTH[name])
    a.n, a.rays_per_lane = n, rays_per_lane
    counters = None
    if count_tests is not None:
        counters = torch.zeros(abi.COUNTERS_WORDS, dtype=torch.int64, device="cuda")
        a.counters, a.count_tests = counters.data_ptr(), count_tests
    rc = lib().rt_occluded_rays(ds.handle, C.byref(a), C.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0, (rc, lib().rt_last_error())
    torch.cuda.synchronize()
    out = {}
    for name in outputs:
        raw = bufs[name].cpu().numpy().reshape(n + 2 * GUARD, WIDTH[name])
        assert np.all(raw[:GUARD] == FILL) and np.all(raw[n + GUARD:] == FILL), name
        body = raw[GUARD:n + GUARD].copy()
        out[name] = body.reshape(n) if name == "occluded" else body.view(np.int32).reshape(n)
    if counters is not None:
        out["counters"] = counters.cpu().numpy()
    return out


def same_bits(a: dict, b: dict, n: int | None = None) -> None:
    for name in ("occluded", "blocker"):
        if name in a and name in b:
            assert a[name][:n].tobytes() == b[name][:n].tobytes(), name


def consistent(got: dict, scene) -> None:
    """occluded is 0 or 1; blocker is -1 exactly where it is 0, and otherwise the index of an active hittable."""
    occ, blk = got["occluded"], got["blocker"]
    assert np.all((occ == 0) | (occ == 1))
    assert np.array_equal(blk == -1, occ == 0)
    assert np.all(blk[occ == 1] >= 0) and blk.max(initial=-1) < scene.num_hittables
    assert all(scene.hittables[int(b)].is_active for b in np.unique(blk[occ == 1]))


def trace_rays(ds: DeviceScene, rays: torch.Tensor, n: int, count_tests: int = 0) -> tuple:
    hits = torch.full((n, 2), -7, dtype=torch.int32, device="cuda")
    counters = torch.zeros(abi.COUNTERS_WORDS, dtype=torch.int64, device="cuda")
    assert lib().rt_trace_rays(ds.handle, C.c_void_p(rays.data_ptr()), n, C.c_void_p(hits.data_ptr()),
                               C.c_void_p(counters.data_ptr()), count_tests,
                               C.c_void_p(torch.cuda.current_stream().cuda_stream)) == 0, lib().rt_last_error()
    torch.cuda.synchronize()
    return hits.cpu().numpy(), counters.cpu().numpy()


def with_range(rays: np.ndarray, tmin, tmax) -> torch.Tensor:
    r = np.array(rays, dtype=F)
    r[:, 0, 3], r[:, 1, 3] = tmin, tmax
    return torch.from_numpy(r).cuda()


@pytest.mark.parametrize("scene", ["rtiow", "wide"])
@pytest.mark.parametrize("camera,size", FRAMES)
def test_against_the_closest_hit(scene, camera, size):
    """Check 1, on every ray: over (0.001, FLT_MAX) a ray is occluded exactly when rt_trace_rays finds a hit; cut off at
    half the closest hit's distance nothing is hit, at twice the distance something is.  Both follow from the traversal
    (a box the closest-hit traversal passed with its t_best >= t is passed with tmax = 2t, and nothing lies before t):
    a failure is a bug, not rounding."""
    ref = query_case(scene, camera, size)
    ds, desc = device_scene(scene), query_scene(scene)
    n = ref["rays"].shape[0]
    rays = with_range(ref["rays"], 0.001, FLT_MAX)
    hits, _ = trace_rays(ds, rays, n)
    hit = hits[:, 0] >= 0
    got = occluded(ds, rays, n)
    consistent(got, desc)
    assert np.array_equal(got["occluded"] == 1, hit), np.nonzero((got["occluded"] == 1) != hit)[0][:8]
    t = hits[:, 1].copy().view(F)
    for factor, want in ((0.5, 0), (2.0, 1)):
        tmax = np.full(n, FLT_MAX, dtype=F)
        tmax[hit] = F(factor) * t[hit]
        cut = occluded(ds, with_range(ref["rays"], 0.001, tmax), n)
        consistent(cut, desc)
        assert np.all(cut["occluded"][hit] == want), (factor, np.nonzero(cut["occluded"][hit] != want)[0][:8])
        assert not cut["occluded"][~hit].any()
    print(f"{scene} {camera} {size[0]}x{size[1]}: occluded {hit.mean():.3f}")


@pytest.mark.parametrize("scene,camera,size", SHADOW_FRAMES)
def test_against_the_reference(scene, camera, size):
    """Check 2: shadow rays towards a point light inside the scene, range (0.001, 1).  On decidable rays `occluded` is
    the reference's; each of their blockers is hit within the ray's range by the oracle's own test."""
    case = shadow_case(scene, camera, size)
    ds, desc = device_scene(scene), query_scene(scene)
    n = case["rays"].shape[0]
    got = occluded(ds, torch.from_numpy(case["rays"].copy()).cuda(), n)
    consistent(got, desc)
    dec = case["decidable"]
    share = 1.0 - float(dec.mean())
    occ = got["occluded"] == 1
    wrong = dec & (occ != case["occluded"])
    print(f"{scene} {camera} {size[0]}x{size[1]}: undecidable {share:.4f}, occluded {occ.mean():.3f} "
          f"(reference {case['occluded'].mean():.3f}), differing undecidable rays {int((~dec & (occ != case['occluded'])).sum())}")
    assert share <= UNDECIDABLE_CAP, share
    assert not wrong.any(), (int(wrong.sum()), np.nonzero(wrong)[0][:8])
    rays = case["rays"]
    for r in np.nonzero(dec & occ)[0]:
        h = desc.hittables[int(got["blocker"][r])]
        assert hittable_hits(h, rays[r, 0, :3], rays[r, 1, :3], rays[r, 0, 3], rays[r, 1, 3]), (r, int(got["blocker"][r]))
    if scene == "wide" and camera == "far":  # (the upper reference bits are exercised)
        bvh_index = np.argsort(prim_source(scene))  # hittable index -> index in BVH order (active hittables)
        src = prim_source(scene)
        assert np.array_equal(src[bvh_index[src]], src)
        top = int(bvh_index[got["blocker"][occ]].max())
        print(f"largest BVH index among the blockers {top}")
        assert top >= 8192, top


@pytest.mark.parametrize("kind", ["rect", "sphere"])
def test_hand_made_ranges(kind):
    """Check 3: closed ends for the rectangle, open ends and the far root for the sphere, empty and NaN ranges — exact
    expected values (tests/test_occlusion_host.py derives them from the oracle's own test)."""
    scene = one_primitive_scene(kind)
    ds = DeviceScene(scene)
    rays, expected = hand_rays(kind)
    back = rays[:3].copy()  # ranges behind the origin: the rectangle at t = -1, the sphere's roots at -4 and -2
    back[:, 1, 2] = 1.0
    back[:, 0, 3], back[:, 1, 3] = (-5.0, -1.0, -1.5), (-0.5, 5.0, -1.25)
    rays = np.concatenate([rays, back])
    expected = np.concatenate([expected, occlusion_reference(scene, back, prefilter=False)])
    got = occluded(ds, torch.from_numpy(rays).cuda(), rays.shape[0])
    consistent(got, scene)
    assert np.array_equal(got["occluded"] == 1, expected), (kind, got["occluded"], expected)
    assert np.all(got["blocker"][expected] == 0)
    ds.close()


def test_empty_and_inactive_scenes_occlude_nothing():
    rays = with_range(query_case("rtiow", "near", (37, 21))["rays"], 0.001, FLT_MAX)
    three = scenes.builtin(scenes.SCENE_THREE_SPHERES)
    empty = scenes.Scene((abi.HittableDesc * 0)(), three.materials, [])
    for h in three.hittables:
        h.is_active = 0
    for s in (empty, three):
        ds = DeviceScene(s)
        got = occluded(ds, rays, 100)
        assert not got["occluded"].any() and np.all(got["blocker"] == -1)
        ds.close()


def test_schedule_independence_and_batch_edges():
    """Check 4: the range never shrinks, so a lane's visits depend on its ray alone — both outputs are the same bytes
    for every rays_per_lane, regeneration threshold, call, batch size and subset of outputs."""
    case = shadow_case("rtiow", "near", (40, 24))
    ds = device_scene("rtiow")
    # 65 more rays: n = 1025 with 16 rays per lane gives a second wave one ray
    rays = torch.from_numpy(np.concatenate([case["rays"], case["rays"][:65]])).cuda()
    whole = occluded(ds, rays, 960)
    assert 0.2 < whole["occluded"].mean() < 0.8
    for rpl in (0, 1, 3, 16):
        same_bits(occluded(ds, rays, 960, rays_per_lane=rpl), whole)
    same_bits(occluded(ds, rays, 960), whole)
    for threshold in (1, 64):
        prev = lib().rt_set_tuning(abi.RT_TUNE_REGEN_THRESHOLD, threshold)
        try:
            for rpl in (0, 3):
                same_bits(occluded(ds, rays, 960, rays_per_lane=rpl), whole)
        finally:
            lib().rt_set_tuning(abi.RT_TUNE_REGEN_THRESHOLD, prev)
    for leaf_break in (0, 64):
        prev = lib().rt_set_tuning(abi.RT_TUNE_LEAF_BREAK, leaf_break)
        try:
            same_bits(occluded(ds, rays, 960, rays_per_lane=3), whole)
        finally:
            lib().rt_set_tuning(abi.RT_TUNE_LEAF_BREAK, prev)
    full = occluded(ds, rays, 1025, rays_per_lane=16)
    same_bits(full, whole, 960)
    same_bits({k: v[960:] for k, v in full.items()}, whole, 65)  # (the appended rays are the first 65 again)
    for n in (1, 63, 64, 65, 1025):
        same_bits(occluded(ds, rays, n, rays_per_lane=16), full, n)
    for only in ("occluded", "blocker"):
        alone = occluded(ds, rays, 960, outputs=(only,), rays_per_lane=3)
        assert set(alone) == {only}
        same_bits(alone, whole)


def test_counters():
    """Check 5: counters[0] counts the rays that start a traversal — a ray refused by !(tmin <= tmax) does not count —
    and stopping at the first hit tests no more boxes and primitives than the closest-hit call does for the same rays."""
    ref = query_case("rtiow", "near", (40, 24))
    ds = device_scene("rtiow")
    r = np.array(ref["rays"], dtype=F)
    r[:, 0, 3], r[:, 1, 3] = 0.001, FLT_MAX
    refused = [5, 64, 200, 333, 959]
    r[refused[0], 1, 3] = 0.0005              # tmax < tmin
    r[refused[1], 0, 3] = np.nan
    r[refused[2], 1, 3] = np.nan
    r[refused[3], 0, 3], r[refused[3], 1, 3] = 2.0, 1.0
    r[refused[4], 0, 3], r[refused[4], 1, 3] = np.inf, -np.inf
    n = r.shape[0]
    for count_tests in (0, 1):
        got = occluded(ds, torch.from_numpy(r).cuda(), n, count_tests=count_tests)
        assert int(got["counters"][0]) == n - len(refused), got["counters"][:4]
        assert not got["occluded"][refused].any() and np.all(got["blocker"][refused] == -1)
        if not count_tests:
            assert not got["counters"][1:3].any()
    rays = with_range(ref["rays"], 0.001, FLT_MAX)
    occ = occluded(ds, rays, n, count_tests=1)["counters"]
    hits, clo = trace_rays(ds, rays, n, count_tests=1)
    assert int(occ[0]) == n == int(clo[0])
    print(f"box tests per ray {occ[1] / n:.2f} (closest hit {clo[1] / n:.2f}), primitive tests per ray {occ[2] / n:.2f} "
          f"(closest hit {clo[2] / n:.2f}), summed ratio {(occ[1] + occ[2]) / (clo[1] + clo[2]):.3f}")
    assert occ[1] > 0 and occ[2] > 0
    assert occ[1] + occ[2] <= clo[1] + clo[2], (occ[1:3], clo[1:3])


def test_device_scene_occluded_equals_the_direct_call():
    """Check 6: DeviceScene.occluded from a numpy array and from a device tensor."""
    case = shadow_case("wide", "far", (37, 21))
    ds = device_scene("wide")
    n = case["rays"].shape[0]
    rays = torch.from_numpy(case["rays"].copy()).cuda()
    direct = occluded(ds, rays, n)
    for given in (case["rays"], rays):
        occ = ds.occluded(given)
        torch.cuda.synchronize()
        assert isinstance(occ, torch.Tensor) and occ.dtype == torch.bool and tuple(occ.shape) == (n,)
        assert np.array_equal(occ.cpu().numpy(), direct["occluded"] == 1)
        occ, blk = ds.occluded(given, blocker=True, rays_per_lane=2)
        torch.cuda.synchronize()
        assert occ.dtype == torch.bool and blk.dtype == torch.int32 and tuple(blk.shape) == (n,)
        assert np.array_equal(occ.cpu().numpy(), direct["occluded"] == 1)
        assert blk.cpu().numpy().tobytes() == direct["blocker"].tobytes()
    empty = ds.occluded(rays[:0])
    assert empty.dtype == torch.bool and tuple(empty.shape) == (0,)
    occ, blk = ds.occluded(rays[:0], blocker=True)
    assert tuple(occ.shape) == (0,) and tuple(blk.shape) == (0,) and blk.dtype == torch.int32
    with pytest.raises(ValueError):
        ds.occluded(rays.reshape(-1, 4))
