"""The per-ray entry points' outputs do not depend on the schedule (GPU).

rt_trace_rays, rt_query_rays, rt_occluded_rays, rt_radiance_rays (with and without RT_RADIANCE_DIRECT_LIGHT),
rt_adaptive_samples and rt_temporal_gradient run one work-list schedule (ray_wave_run in render.hip; the kernels of
rt_query_rays and rt_occluded_rays run it from copies of their own, which a change to it must reach too): a wave owns
64 · rays_per_lane consecutive items and a lane that finishes takes the wave's next one, so which lane traces which item
depends on rays_per_lane and on the traversals' lengths.  Every kernel promises that its result does not: here the
outputs must be bit-identical across rays_per_lane 1, 3 and 16, for 1 item, a partial wave (63), a second wave holding
one item (65) and a 16-per-lane range plus one (64 · 16 + 1).  rt_trace_rays has only the automatic setting; it is
compared with rt_query_rays' `hits`.

The scene is c5, the smallest built-in one whose BVH has more than one level (two nodes over five primitives; c1 is a
single node); the direct-light kernel runs on c3, the Cornell box, which has one sampled light.  No reference is
computed: the direct calls of the features' own GPU tests, their guards included, are compared with each other."""
from __future__ import annotations

import ctypes as C
import functools

import numpy as np
import pytest
import torch

from cudaraytracer_amd import abi
from cudaraytracer_amd._lib import lib

from test_direct_light_host import DIRECT, lights_of
from test_gpu_adaptive import adaptive, same_planes
from test_gpu_occlusion import occluded
from test_gpu_occlusion import same_bits as same_occlusion
from test_gpu_query import query, trace_rays
from test_gpu_query import same_bits as same_records
from test_gpu_radiance import GUARD, _body, _guarded, _stream, camera, device_scene, radiance
from test_gpu_radiance import same_bits as same_radiance
from test_radiance_host import FRAMES, SEED, frame_inputs, frame_scene

pytestmark = pytest.mark.gpu

F = np.float32
COUNTS = [1, 63, 65, 64 * 16 + 1]
LANES = (1, 3, 16)
OUT_BYTES = {"gradient": 8, "resample": 16, "pixel": 4}
# (w, h) with w · h strata at stride 1
GRADIENT_FRAMES = {1: (1, 1), 63: (9, 7), 65: (13, 5), 64 * 16 + 1: (41, 25)}


@functools.lru_cache(maxsize=None)
def rays_of(name: str) -> torch.Tensor:
    """At least 64 · 16 + 1 rays into the frame's scene: its Philox-jittered camera rays from the middle row on (so that
    the first few meet the scene), then the whole frame's."""
    rays, _ = camera(name, "philox", 0)
    rays = torch.cat([rays[rays.shape[0] // 2:], rays])
    assert rays.shape[0] >= COUNTS[-1]
    return rays.contiguous()


def planes_of(n_pixels: int) -> dict:
    """History, moments and accumulation planes with a different value in every pixel."""
    i = np.arange(n_pixels, dtype=F)
    hist = np.stack([0.25 + i / 4096.0, 0.5 - i / 8192.0, 0.125 + i / 2048.0, 1.0 + (i % 5)], axis=1).astype(F)
    lum = (0.2126 * hist[:, 0] + 0.7152 * hist[:, 1] + 0.0722 * hist[:, 2]).astype(F)
    return {"history": hist, "moments": np.stack([lum, lum * lum + F(0.01)], axis=1).astype(F),
            "accum": np.stack([hist[:, 0], hist[:, 1], hist[:, 2], np.full(n_pixels, 3.0, dtype=F)], axis=1).astype(F)}


def gradient(name: str, size, k: int, rays_per_lane: int, depth: int | None = None) -> dict:
    """One rt_temporal_gradient call at stride 1 on a frame of `size` under the camera of frame `name`."""
    w, h = size
    n = w * h
    i = np.arange(n, dtype=F)
    prev = torch.from_numpy(np.stack([i / 2048.0, 0.5 + i / 4096.0, 1.0 - i / 4096.0, np.full(n, 7.5, dtype=F)], axis=1)
                            .astype(F)).cuda()
    a = abi.TemporalGradientArgs()
    a.prev_color = prev.data_ptr()
    bufs = {}
    for o, width in OUT_BYTES.items():
        bufs[o] = _guarded(n, width)
        setattr(a, o, bufs[o].data_ptr() + GUARD * width)
    a.width, a.height, a.stride, a.offset_x, a.offset_y = w, h, 1, 0, 0
    a.samples_per_pixel, a.rays_per_lane, a.flags = k, rays_per_lane, 0
    a.max_depth = FRAMES[name][3] if depth is None else depth
    a.rng_seed, a.rng_frame = SEED, 0
    a.tiling = abi.Tiling(h, 1, 0, h)
    a.inputs = frame_inputs(name)
    rc = lib().rt_temporal_gradient(device_scene(name).handle, C.byref(a), _stream())
    assert rc == 0, (rc, lib().rt_last_error())
    torch.cuda.synchronize()
    return {o: _body(bufs[o], n, width, o) for o, width in OUT_BYTES.items()}


def same_gradient(a: dict, b: dict) -> None:
    for o in OUT_BYTES:
        assert a[o].tobytes() == b[o].tobytes(), o


def each_schedule(call, same) -> list:
    """call(rays_per_lane) for 1, 3 and 16; every result must equal the first."""
    results = [call(rpl) for rpl in LANES]
    for r in results[1:]:
        same(results[0], r)
    return results


def test_the_scenes_are_what_the_cases_need():
    info = abi.HostTablesInfo()
    assert lib().rt_build_host_tables(C.byref(frame_scene("c5").desc()), None, None, None, None, C.byref(info)) == 0
    assert info.num_nodes > 1
    assert lights_of(frame_scene("c3"))[0] == 1


@pytest.mark.parametrize("n", COUNTS)
def test_closest_hit_queries(n):
    """rt_query_rays across rays_per_lane, every record; rt_trace_rays against its `hits`."""
    ds, rays = device_scene("c5"), rays_of("c5")
    results = each_schedule(lambda rpl: query(ds, rays, n, rays_per_lane=rpl), same_records)
    assert trace_rays(ds, rays, n).tobytes() == results[0]["hits"].tobytes()
    if n == COUNTS[-1]:  # (not a frame of sky)
        assert np.any(results[0]["hits"][:, 0] >= 0)


@pytest.mark.parametrize("n", COUNTS)
def test_occlusion(n):
    ds = device_scene("c5")
    r = rays_of("c5").clone()
    r[:, 0, 3], r[:, 1, 3] = 1e-3, 1e30
    r[::7, 1, 3] = -1.0  # (an empty range: stored without a traversal)
    each_schedule(lambda rpl: occluded(ds, r, n, rays_per_lane=rpl), same_occlusion)


@pytest.mark.parametrize("n", COUNTS)
def test_radiance(n):
    ds, rays = device_scene("c5"), rays_of("c5")
    each_schedule(lambda rpl: radiance(ds, "c5", rays, n, samples=2, rays_per_lane=rpl), same_radiance)


@pytest.mark.parametrize("n", COUNTS)
def test_direct_light(n):
    ds, rays = device_scene("c3"), rays_of("c3")
    results = each_schedule(lambda rpl: radiance(ds, "c3", rays, n, samples=2, flags=DIRECT, rays_per_lane=rpl), same_radiance)
    if n == COUNTS[-1]:  # (the flag does something here: a light is sampled)
        plain = radiance(ds, "c3", rays, n, samples=2)
        assert plain["sum"].tobytes() != results[0]["sum"].tobytes()


@pytest.mark.parametrize("n", COUNTS)
def test_adaptive_samples(n):
    w, h = FRAMES["c5"][2]
    planes = planes_of(w * h)
    pixels = (np.arange(n, dtype=np.int64) * 977) % (w * h)  # (977 and 1536 are coprime: every pixel at most once)
    samples = 1 + np.arange(n) % 3
    each_schedule(lambda rpl: adaptive("c5", pixels, planes, samples=samples, rays_per_lane=rpl), same_planes)


def test_adaptive_samples_invalid_entries_and_device_count():
    w, h = FRAMES["c5"][2]
    planes = planes_of(w * h)
    outside = w * h + np.arange(32)
    # 64 invalid entries (32 pixels outside the frame, 32 with 0 samples), then one valid one
    pixels = np.concatenate([outside, np.arange(32), [700]])
    samples = np.concatenate([np.full(32, 2), np.zeros(32, dtype=np.int64), [2]])
    tail = each_schedule(lambda rpl: adaptive("c5", pixels, planes, samples=samples, rays_per_lane=rpl), same_planes)
    alone = adaptive("c5", [700], planes, samples=[2])
    same_planes(tail[0], alone)
    assert tail[0]["history"][700].tobytes() != planes["history"][700].tobytes()
    # only invalid entries: nothing is written
    none = each_schedule(lambda rpl: adaptive("c5", pixels[:64], planes, samples=samples[:64], rays_per_lane=rpl), same_planes)
    same_planes(none[0], planes)
    # a device count below the capacity: the entries beyond it are not run
    pixels = (np.arange(200, dtype=np.int64) * 977) % (w * h)
    counted = each_schedule(lambda rpl: adaptive("c5", pixels, planes, count=[70], spp=2, rays_per_lane=rpl), same_planes)
    same_planes(counted[0], adaptive("c5", pixels[:70], planes, spp=2))


@pytest.mark.parametrize("n", COUNTS)
def test_temporal_gradient(n):
    each_schedule(lambda rpl: gradient("c5", GRADIENT_FRAMES[n], 2, rpl), same_gradient)


def test_depth_zero_with_two_samples():
    """max_depth 0: every sample is 0 and nothing is traced, in all four path kernels."""
    n = 65
    for name, flags in (("c5", 0), ("c3", DIRECT)):
        ds, rays = device_scene(name), rays_of(name)
        got = each_schedule(lambda rpl: radiance(ds, name, rays, n, samples=2, depth=0, flags=flags, rays_per_lane=rpl,
                                                 count_tests=1), same_radiance)
        assert not np.any(got[0]["sum"][:, :3]) and not np.any(got[0]["mean"][:, :3])
        assert all(int(g["counters"][0]) == 0 for g in got)
    w, h = FRAMES["c5"][2]
    planes = planes_of(w * h)
    pixels = (np.arange(n, dtype=np.int64) * 977) % (w * h)
    got = each_schedule(lambda rpl: adaptive("c5", pixels, planes, spp=2, depth=0, rays_per_lane=rpl, count_tests=1), same_planes)
    assert got[0]["accum"][pixels, :3].tobytes() == planes["accum"][pixels, :3].tobytes()
    assert np.all(got[0]["accum"][pixels, 3] == planes["accum"][pixels, 3] + F(2.0))
    assert all(int(g["counters"][0]) == 0 for g in got)
    got = each_schedule(lambda rpl: gradient("c5", GRADIENT_FRAMES[n], 2, rpl, depth=0), same_gradient)
    assert not np.any(got[0]["resample"].view(F).reshape(n, 4)[:, :3])
