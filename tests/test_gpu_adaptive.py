"""rt_adaptive_select and rt_adaptive_samples on the GPU.

Frames, scenes and the oracle's samples are those of tests/test_radiance_host.py; the selection rule and the merges are
the numpy restatements of tests/test_adaptive_host.py.  Every call goes to the C entry points directly (but for the last
test, which goes through Renderer.adaptive), with the outputs — the planes that are merged in place included — inside
buffers filled with 0x5a, 16 guard elements before and after each, checked after the call.  Everything is compared bit
for bit."""
from __future__ import annotations

import ctypes as C

import numpy as np
import pytest
import torch

from cudaraytracer_amd import abi
from cudaraytracer_amd._lib import lib
from cudaraytracer_amd.renderer import Renderer

from test_adaptive_host import merge_accum, merge_history, reset_planes, select_reference, synthetic_planes
from test_gpu_radiance import FILL, GUARD, _body, _guarded, _stream, camera, device_scene, radiance
from test_radiance_host import FRAMES, SEED, frame_inputs, sample_reference

pytestmark = pytest.mark.gpu

F = np.float32
PLANE_BYTES = {"history": 16, "moments": 8, "accum": 16}


def _u32(values) -> torch.Tensor:
    return torch.from_numpy(np.asarray(values, dtype=np.uint32).view(np.int32).copy()).cuda()


# ---------------------------------------------------------------------------------------------------------------------
# Direct calls
# ---------------------------------------------------------------------------------------------------------------------
def select(history, moments, prim_id, w, h, capacity, pixels_per_lane=0, with_samples=True, **params) -> tuple:
    """One rt_adaptive_select call on numpy planes: (pixels body (capacity,), samples body (capacity,) — both still
    holding the fill where nothing was written — and count (2,)), after checking the guards."""
    n = w * h
    dev = {"history": torch.from_numpy(np.ascontiguousarray(history, dtype=F)).cuda(),
           "moments": torch.from_numpy(np.ascontiguousarray(moments, dtype=F)).cuda()}
    if prim_id is not None:
        dev["prim_id"] = torch.from_numpy(np.ascontiguousarray(prim_id, dtype=np.int32)).cuda()
    a = abi.AdaptiveSelectArgs()
    for name, t in dev.items():
        setattr(a, name, t.data_ptr())
    pixels, samples, count = _guarded(capacity, 4), _guarded(capacity, 4), _guarded(2, 4)
    a.pixels = pixels.data_ptr() + GUARD * 4
    if with_samples:
        a.samples = samples.data_ptr() + GUARD * 4
    a.count = count.data_ptr() + GUARD * 4
    scratch = torch.full((int(lib().rt_adaptive_select_scratch_bytes(w, h)),), FILL, dtype=torch.uint8, device="cuda")
    a.scratch = scratch.data_ptr()
    a.width, a.height, a.capacity, a.pixels_per_lane = w, h, capacity, pixels_per_lane
    a.max_samples, a.min_history = params["max_samples"], params["min_history"]
    a.tau, a.lum_floor = params["tau"], params["lum_floor"]
    a.tiling = abi.Tiling(max(h, 1), 1, 0, h)
    rc = lib().rt_adaptive_select(C.byref(a), _stream())
    assert rc == 0, (rc, lib().rt_last_error())
    torch.cuda.synchronize()
    return (_body(pixels, capacity, 4, "pixels").view(np.uint32).reshape(capacity),
            _body(samples, capacity, 4, "samples").view(np.uint32).reshape(capacity),
            _body(count, 2, 4, "count").view(np.uint32).reshape(2))


def adaptive(name, pixels, planes: dict, samples=None, count=None, base=1, spp=1, max_samples=16, max_history=32,
             flags=0, rays_per_lane=0, count_tests=0, depth=None) -> dict:
    """One rt_adaptive_samples call on the frame `name`: `planes` maps history / moments / accum to their initial
    (W·H, c) float32 contents; returns the planes after the call and "counters", after checking the guards."""
    w, h = FRAMES[name][2]
    n = w * h
    ds = device_scene(name)
    a = abi.AdaptiveSamplesArgs()
    keep = [_u32(pixels)]
    a.pixels = keep[0].data_ptr()
    if samples is not None:
        keep.append(_u32(samples))
        a.samples = keep[-1].data_ptr()
    if count is not None:
        keep.append(_u32(count))
        a.count = keep[-1].data_ptr()
    bufs = {}
    for o, init in planes.items():
        bufs[o] = _guarded(n, PLANE_BYTES[o])
        body = torch.from_numpy(np.ascontiguousarray(init, dtype=F).view(np.uint8).reshape(-1)).cuda()
        bufs[o][GUARD * PLANE_BYTES[o]:(GUARD + n) * PLANE_BYTES[o]] = body
        setattr(a, o, bufs[o].data_ptr() + GUARD * PLANE_BYTES[o])
    counters = torch.zeros(abi.COUNTERS_WORDS, dtype=torch.int64, device="cuda")
    a.counters, a.count_tests = counters.data_ptr(), count_tests
    a.capacity, a.width, a.height = len(pixels), w, h
    a.samples_per_pixel, a.max_samples, a.sample_base = spp, max_samples, base
    a.max_depth = FRAMES[name][3] if depth is None else depth
    a.max_history, a.rays_per_lane, a.flags = max_history, rays_per_lane, flags
    a.rng_seed, a.rng_frame = SEED, 0
    a.inputs = frame_inputs(name)
    rc = lib().rt_adaptive_samples(ds.handle, C.byref(a), _stream())
    assert rc == 0, (rc, lib().rt_last_error())
    torch.cuda.synchronize()
    out = {o: _body(bufs[o], n, PLANE_BYTES[o], o).view(F).reshape(n, PLANE_BYTES[o] // 4) for o in planes}
    out["counters"] = counters.cpu().numpy()
    return out


def start_planes(name: str) -> dict:
    """The three planes as sample 0 of the oracle's frame leaves them: accum (q_0 / 4096, 1); history (c_0, 1) and moments
    (l, l·l), a reset pass's."""
    q0, _ = sample_reference(name, 0)
    hist, mom = reset_planes(q0)
    return {"accum": hist.copy(), "history": hist, "moments": mom}


def same_planes(a: dict, b: dict, rows=None) -> None:
    for o in PLANE_BYTES:
        if o in a and o in b:
            assert (a[o] if rows is None else a[o][rows]).tobytes() == (b[o] if rows is None else b[o][rows]).tobytes(), o


# ---------------------------------------------------------------------------------------------------------------------
SELECT_PARAMS = dict(tau=0.15, lum_floor=0.01, min_history=4, max_samples=8)


@pytest.mark.parametrize("size", [(37, 21), (40, 24), (65, 33)])
def test_select_equals_the_rule(size):
    """pixels, samples and count against the numpy rule: a list that fits, one that is cut, one of a single entry and an
    all-miss frame, each under three launch shapes (1, 4 and 16 pixels per lane: 9, 3 and 1 workgroups at 65 x 33)."""
    w, h = size
    n = w * h
    hist, mom, pid = synthetic_planes(w, h, seed=w)
    want_p, want_k, want_c = select_reference(hist[:, 3], mom, pid, **SELECT_PARAMS)
    total = int(want_c[0])
    assert 0.05 * n < total < 0.9 * n and len(np.unique(want_k)) > 3
    untouched = np.full(1, FILL * 0x01010101, dtype=np.uint32)[0]
    for ppl in (0, 1, 16):
        for capacity in (n, total, total - 7, 1):
            got_p, got_k, got_c = select(hist, mom, pid, w, h, capacity, ppl, **SELECT_PARAMS)
            m = min(total, capacity)
            assert np.array_equal(got_c, want_c), (ppl, capacity, got_c, want_c)
            assert np.array_equal(got_p[:m], want_p[:m]) and np.array_equal(got_k[:m], want_k[:m]), (ppl, capacity)
            assert np.all(got_p[m:] == untouched) and np.all(got_k[m:] == untouched), (ppl, capacity)
        # without the samples output, and without prim_id (every pixel valid)
        got_p, got_k, got_c = select(hist, mom, pid, w, h, n, ppl, with_samples=False, **SELECT_PARAMS)
        assert np.array_equal(got_p[:total], want_p) and np.all(got_k == untouched) and np.array_equal(got_c, want_c)
        all_p, all_k, all_c = select_reference(hist[:, 3], mom, None, **SELECT_PARAMS)
        got_p, got_k, got_c = select(hist, mom, None, w, h, n, ppl, **SELECT_PARAMS)
        assert np.array_equal(got_c, all_c) and np.array_equal(got_p[:all_c[0]], all_p) and np.array_equal(got_k[:all_c[0]], all_k)
        # an all-miss frame: count 0, the list untouched
        got_p, got_k, got_c = select(hist, mom, np.full(n, -1, dtype=np.int32), w, h, n, ppl, **SELECT_PARAMS)
        assert not got_c.any() and np.all(got_p == untouched) and np.all(got_k == untouched)
    # an empty list: count alone is written; an empty frame: (0, 0)
    a = abi.AdaptiveSelectArgs()
    dev = [torch.from_numpy(x).cuda() for x in (hist, mom)]
    count = torch.full((2,), 77, dtype=torch.int32, device="cuda")
    scratch = torch.zeros(int(lib().rt_adaptive_select_scratch_bytes(w, h)), dtype=torch.uint8, device="cuda")
    a.history, a.moments, a.count, a.scratch = dev[0].data_ptr(), dev[1].data_ptr(), count.data_ptr(), scratch.data_ptr()
    a.width, a.height, a.max_samples, a.min_history, a.tau, a.lum_floor = w, h, 8, 4, 0.15, 0.01
    assert lib().rt_adaptive_select(C.byref(a), _stream()) == 0, lib().rt_last_error()
    torch.cuda.synchronize()
    assert count.cpu().numpy().view(np.uint32).tolist() == select_reference(hist[:, 3], mom, None, **SELECT_PARAMS)[2].tolist()
    a.height = 0
    assert lib().rt_adaptive_select(C.byref(a), _stream()) == 0, lib().rt_last_error()
    torch.cuda.synchronize()
    assert count.cpu().tolist() == [0, 0]


@pytest.mark.parametrize("name", list(FRAMES))
def test_oracle_parity(name):
    """Every pixel listed, 1 and 2 samples alternating along the list from sample 1 on: the accumulation plane ends as
    the oracle's sums of samples 0..k with w = 1 + k, history and moments as the numpy blend of the oracle's samples
    1..k onto a reset pass's planes, with max_history 32 and with 2, where the cap bites.  The complementary list (2 and
    1 alternating) likewise, and the two launches together trace the rays the oracle counts for two frames' sample 1
    and one frame's sample 2.  (c2 37x21: under both Random() fill orders.)"""
    w, h = FRAMES[name][2]
    n = w * h
    pixels = np.arange(n, dtype=np.uint32)
    orders = ((0, 1), (abi.RT_FLAG_RIUS_LEFT_TO_RIGHT, 0)) if name == "c2_37x21" else ((0, 1),)
    for flags, rius in orders:
        q = [sample_reference(name, s, rius_order=rius) for s in range(3)]
        hist0, mom0 = reset_planes(q[0][0])
        begin = {"accum": hist0.copy(), "history": hist0, "moments": mom0}
        traced = 0
        for first in (1, 2):
            k = np.where(pixels % 2 == 0, first, 3 - first).astype(np.uint32)
            two = k == 2
            units = q[1][0].astype(np.uint64) + np.where(two[:, None], q[2][0], 0).astype(np.uint64)
            want_accum = merge_accum(begin["accum"], units, k)
            exact = (q[0][0].astype(np.float64) + units) / 4096.0  # the oracle's own sum of samples 0..k
            assert np.array_equal(want_accum[:, :3].astype(np.float64), exact) and np.array_equal(want_accum[:, 3], 1 + k)
            for max_history in (32, 2):
                hw, mw = merge_history(hist0, mom0, q[1][0], max_history)
                h2, m2 = merge_history(hw, mw, q[2][0], max_history)
                hw[two], mw[two] = h2[two], m2[two]
                got = adaptive(name, pixels, begin, samples=k, flags=flags, max_history=max_history)
                wrong = np.nonzero(np.any(got["accum"] != want_accum, axis=1))[0]
                print(f"{name} flags {flags} first {first} max_history {max_history}: rays {int(got['counters'][0])}, "
                      f"differing pixels {len(wrong)}")
                assert len(wrong) == 0, (len(wrong), wrong[:8], got["accum"][wrong[:4]], want_accum[wrong[:4]])
                assert got["history"].tobytes() == hw.tobytes() and got["moments"].tobytes() == mw.tobytes()
                assert np.all(got["history"][:, 3] == (F(2.0) if max_history == 2 else F(1.0) + k.astype(F)))
                assert int(got["counters"][3]) == int(k.sum())
            traced += int(got["counters"][0])
        assert traced == 2 * q[1][1] + q[2][1], (traced, q[1][1], q[2][1])


def test_one_sample_equals_the_three_step_path():
    """k = 1 on every third pixel: the accumulation plane equals rt_camera_rays(pixels, sample 1) + rt_radiance_rays(sum,
    sample_base 1) + the addition; unlisted pixels, and the pixels of entries with k = 0, keep their bits; entries with an
    index at or beyond W·H touch nothing."""
    name = "c2_37x21"
    w, h = FRAMES[name][2]
    n = w * h
    begin = start_planes(name)
    third = np.arange(0, n, 3, dtype=np.uint32)
    rays, index = camera(name, "philox", 1, pixels=_u32(third))
    parent = radiance(device_scene(name), name, rays, len(third), ids=index, base=1, outputs=("sum",))
    want = {o: v.copy() for o, v in begin.items()}
    want["accum"][third] = (begin["accum"][third] + parent["sum"]).astype(F)
    hw, mw = merge_history(begin["history"][third], begin["moments"][third], parent["q"].astype(np.uint32), 32)
    want["history"][third], want["moments"][third] = hw, mw
    # the list: the third pixels in ascending order, with strangers among them
    pixels = np.concatenate([third[:50], [n, 0xffffffff, 1, 4], third[50:], [n + 5, 7]]).astype(np.uint32)
    samples = np.concatenate([np.ones(50), [1, 1, 0, 0], np.ones(len(third) - 50), [2, 0]]).astype(np.uint32)
    got = adaptive(name, pixels, begin, samples=samples)
    same_planes(got, want)
    listed = np.zeros(n, dtype=bool)
    listed[third] = True
    same_planes(got, begin, ~listed)
    assert np.any(got["accum"][listed] != begin["accum"][listed])
    assert int(got["counters"][0]) == int(parent["counters"][0]) and int(got["counters"][3]) == len(third)
    # samples_per_pixel without a samples list, each target alone, and history without moments
    plain = adaptive(name, third, begin, spp=1)
    same_planes(plain, want)
    for only in (("accum",), ("history",), ("history", "moments")):
        same_planes(adaptive(name, third, {o: begin[o] for o in only}), want)


def test_two_samples_are_two_camera_rays():
    """k = 2 equals two k = 1 calls with sample_base 1 and then 2, and differs from the three-step path's
    samples_per_ray = 2, whose second path starts on the first one's camera ray."""
    name = "c2_40x24"
    w, h = FRAMES[name][2]
    n = w * h
    pixels = np.arange(n, dtype=np.uint32)
    begin = start_planes(name)
    both = adaptive(name, pixels, begin, spp=2)
    one = adaptive(name, pixels, begin, spp=1, base=1)
    two = adaptive(name, pixels, {o: one[o] for o in PLANE_BYTES}, spp=1, base=2)
    same_planes(both, two)
    assert int(both["counters"][0]) == int(one["counters"][0]) + int(two["counters"][0])
    assert np.all(both["accum"][:, 3] == 3) and np.all(both["history"][:, 3] == 3)
    # max_samples caps an entry's paths
    same_planes(adaptive(name, pixels, begin, spp=2, max_samples=1), one)
    same_planes(adaptive(name, pixels, begin, samples=np.full(n, 9, dtype=np.uint32), max_samples=2), both)
    # the parent: sample 1's camera rays, two samples each
    rays, index = camera(name, "philox", 1)
    parent = radiance(device_scene(name), name, rays, n, ids=index, base=1, samples=2, outputs=("sum",))
    mine = (both["accum"][:, :3] - begin["accum"][:, :3]).astype(F)  # (exact: multiples of 2^-12 far below 2^24 units)
    assert np.array_equal(one["accum"][:, :3] - begin["accum"][:, :3],
                          radiance(device_scene(name), name, rays, n, ids=index, base=1, outputs=("sum",))["sum"][:, :3])
    differing = np.any(mine != parent["sum"][:, :3], axis=1)
    print(f"pixels whose second sample differs from the three-step path's: {int(differing.sum())} of {n}")
    assert differing.any()


def test_entry_count_is_read_from_the_device():
    """Launched for the whole list, the pass touches the pixels of the first count[0] entries alone — the list's tail
    holds valid indices on purpose; a count beyond the capacity means the capacity."""
    name = "c2_37x21"
    w, h = FRAMES[name][2]
    n = w * h
    begin = start_planes(name)
    pixels = np.random.default_rng(7).permutation(n).astype(np.uint32)[:300]
    whole = adaptive(name, pixels, begin)
    for m in (0, 1, 63, 64, 65, 130):
        got = adaptive(name, pixels, begin, count=[m, 12345])
        head = np.zeros(n, dtype=bool)
        head[pixels[:m]] = True
        same_planes(got, whole, head)
        same_planes(got, begin, ~head)
        assert int(got["counters"][3]) == m
    for m in (300, 301, 0xffffffff):
        same_planes(adaptive(name, pixels, begin, count=[m, 0]), whole)


def test_schedule_independence():
    """rays_per_lane 0, 1 and 16, the counting build, two tunings and a repeated call: the same bits."""
    name = "c2_37x21"
    w, h = FRAMES[name][2]
    n = w * h
    begin = start_planes(name)
    pixels = np.arange(n, dtype=np.uint32)
    samples = (1 + (pixels * 7 + pixels // 5) % 3).astype(np.uint32)  # 1..3 paths, mixed within every wave
    whole = adaptive(name, pixels, begin, samples=samples, base=0)
    same_planes(adaptive(name, pixels, begin, samples=samples, base=0), whole)
    for rpl in (1, 3, 16):
        got = adaptive(name, pixels, begin, samples=samples, base=0, rays_per_lane=rpl)
        same_planes(got, whole)
        assert int(got["counters"][0]) == int(whole["counters"][0])
    counted = adaptive(name, pixels, begin, samples=samples, base=0, count_tests=1)
    same_planes(counted, whole)
    assert int(counted["counters"][0]) == int(whole["counters"][0]) and int(counted["counters"][1]) > 0
    for key, v in ((abi.RT_TUNE_REGEN_THRESHOLD, 1), (abi.RT_TUNE_LEAF_BREAK, 64)):
        prev = lib().rt_set_tuning(key, v)
        try:
            same_planes(adaptive(name, pixels, begin, samples=samples, base=0, rays_per_lane=3), whole)
        finally:
            lib().rt_set_tuning(key, prev)
    # max_depth = 0: every sample is 0 and nothing is traced, but the samples are merged
    dark = adaptive(name, pixels, begin, samples=samples, base=0, depth=0)
    assert int(dark["counters"][0]) == 0 and int(dark["counters"][3]) == int(samples.sum())
    assert np.array_equal(dark["accum"][:, :3], begin["accum"][:, :3]) and np.all(dark["accum"][:, 3] == 1 + samples)
    zero = np.zeros((n, 3), dtype=np.uint32)
    hw, mw = begin["history"], begin["moments"]
    for j in range(3):
        h2, m2 = merge_history(hw, mw, zero, 32)
        more = samples > j
        hw, mw = np.where(more[:, None], h2, hw), np.where(more[:, None], m2, mw)
    assert dark["history"].tobytes() == hw.tobytes() and dark["moments"].tobytes() == mw.tobytes()


def test_renderer_adaptive_end_to_end():
    """A 1-spp Philox frame, gbuffer, a reset temporal(moments=True), then Renderer.adaptive: count and the list are the
    numpy rule's on the planes the pass found; the listed pixels' history and moments are the numpy blend of the oracle's
    samples 1..k; every other pixel keeps its bits."""
    name = "c5"
    w, h = FRAMES[name][2]
    n = w * h
    ds, inp, depth = device_scene(name), frame_inputs(name), FRAMES[name][3]
    r = Renderer(w, h, rng="philox")
    r.render_init(SEED)
    r.render(ds, 1, depth, inp, radiance=True)
    r.gbuffer(ds, inp)
    r.temporal(moments=True)
    torch.cuda.synchronize()
    hist0 = r.history.cpu().numpy().reshape(n, 4).copy()
    mom0 = r.moments.cpu().numpy().reshape(n, 2).copy()
    pid = r.prim_id.cpu().numpy().reshape(n)
    want_h, want_m = reset_planes(sample_reference(name, 0)[0])
    assert hist0.tobytes() == want_h.tobytes() and mom0.tobytes() == want_m.tobytes()  # (the frame is the oracle's sample 0)
    print(f"misses: {int((pid < 0).sum())} of {n}")
    params = dict(tau=0.1, lum_floor=0.01, min_history=3, max_samples=2)
    want_p, want_k, want_c = select_reference(hist0[:, 3], mom0, pid, **params)
    assert np.array_equal(want_p, np.nonzero(pid >= 0)[0]) and np.all(want_k == 2)  # a reset history: N = 1, no variance yet
    for capacity, cut in ((None, len(want_p)), (100, 100)):
        if capacity is not None:  # the planes as they were
            r.history.copy_(torch.from_numpy(hist0.reshape(h, w, 4)).cuda())
            r.moments.copy_(torch.from_numpy(mom0.reshape(h, w, 2)).cuda())
        count = r.adaptive(ds, inp, depth, capacity=capacity, frame=0, seed=SEED, **params)
        torch.cuda.synchronize()
        assert count.cpu().numpy().view(np.uint32).tolist() == want_c.tolist()
        assert np.array_equal(r.adaptive_pixels.cpu().numpy().view(np.uint32)[:cut], want_p[:cut])
        assert np.array_equal(r.adaptive_samples.cpu().numpy().view(np.uint32)[:cut], want_k[:cut])
        hw, mw = hist0, mom0
        for s in (1, 2):
            hw, mw = merge_history(hw, mw, sample_reference(name, s)[0], 32)
        listed = np.zeros(n, dtype=bool)
        listed[want_p[:cut]] = True
        got_h, got_m = r.history.cpu().numpy().reshape(n, 4), r.moments.cpu().numpy().reshape(n, 2)
        assert got_h[listed].tobytes() == hw[listed].tobytes() and got_m[listed].tobytes() == mw[listed].tobytes()
        assert got_h[~listed].tobytes() == hist0[~listed].tobytes() and got_m[~listed].tobytes() == mom0[~listed].tobytes()
        assert np.all(got_h[listed, 3] == 3)
    # the default frame is the one render() drew last, the default seed the renderer's
    r.history.copy_(torch.from_numpy(hist0.reshape(h, w, 4)).cuda())
    r.moments.copy_(torch.from_numpy(mom0.reshape(h, w, 2)).cuda())
    r.adaptive(ds, inp, depth, **params)
    torch.cuda.synchronize()
    full = pid >= 0
    got_h = r.history.cpu().numpy().reshape(n, 4)
    assert got_h[full].tobytes() == hw[full].tobytes() and got_h[~full].tobytes() == hist0[~full].tobytes()
