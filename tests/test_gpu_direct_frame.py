"""RT_RADIANCE_DIRECT_LIGHT in rt_adaptive_samples and rt_temporal_gradient on the GPU.

The reference for every bit-for-bit check is the three-step path that existed before: rt_camera_rays (Philox jitter,
sample s, listed pixels), then rt_radiance_rays with the flag, one sample, sample_base = s and the pixel indices as stream
ids — which tests/test_gpu_direct_light.py ties to a numpy restatement and to quadrature.  Its `sum`, in 2^-12 units, goes
through the numpy merges of tests/test_adaptive_host.py and the mean of tests/test_gradient_host.py.  Every call goes to
the C entry points directly (but for the last tests, which go through the Python wrappers), with the outputs — the planes
merged in place included — inside buffers filled with 0x5a, 16 guard elements before and after each, checked after the
call.  Everything is compared bit for bit; nothing here has a tolerance."""
from __future__ import annotations

import ctypes as C
import functools

import numpy as np
import pytest
import torch

from cudaraytracer_amd import abi, scenes
from cudaraytracer_amd._lib import lib
from cudaraytracer_amd.renderer import DeviceScene, Renderer

from test_adaptive_host import merge_accum, merge_history
from test_direct_light_host import DIRECT, lights_of
from test_gpu_direct_light import _metal_c3, _wide_with_rect, floor_scene
from test_gpu_radiance import GUARD, _body, _guarded, _stream, device_scene
from test_gradient_host import gradient_reference, mean_color, strata_pixels
from test_radiance_host import FRAMES, SEED, frame_inputs, frame_scene

pytestmark = pytest.mark.gpu

F = np.float32
LTR = abi.RT_FLAG_RIUS_LEFT_TO_RIGHT
PLANE_BYTES = {"history": 16, "moments": 8, "accum": 16}
OUT_BYTES = {"gradient": 8, "resample": 16, "pixel": 4}


class Frame:
    """A scene on the device under a camera: what every call below takes."""

    def __init__(self, ds: DeviceScene, inputs: abi.InputStruct, size, depth: int):
        self.ds, self.inputs, self.size, self.depth = ds, inputs, size, depth
        self.n = size[0] * size[1]

    def at(self, size=None, depth=None, ds=None) -> "Frame":
        return Frame(ds or self.ds, self.inputs, size or self.size, self.depth if depth is None else depth)


def named(name: str) -> Frame:
    return Frame(device_scene(name), frame_inputs(name), FRAMES[name][2], FRAMES[name][3])


@functools.lru_cache(maxsize=None)
def floor_frame() -> Frame:
    """Two lamps and a shadowing sphere over a Lambertian floor, seen from above at an angle: 24 x 16, depth 3."""
    inp = scenes.camera_inputs((0.3, 3.0, 2.5), scenes.normalized((-0.3, -3.0, -2.2)), 40.0)
    assert lights_of(floor_scene())[0] == 2
    return Frame(DeviceScene(floor_scene()), inp, (24, 16), 3)


def _u32(values) -> torch.Tensor:
    return torch.from_numpy(np.asarray(values, dtype=np.uint32).view(np.int32).copy()).cuda()


# ---------------------------------------------------------------------------------------------------------------------
# Direct calls
# ---------------------------------------------------------------------------------------------------------------------
def three_step(fr: Frame, pixels, s: int, flags: int = DIRECT, frame: int = 0) -> dict:
    """Sample s of the listed pixels by the calls that were there before: rt_camera_rays, then rt_radiance_rays with one
    sample, sample_base = s and the pixels as stream ids.  {"q": (n, 3) uint64 2^-12 units, "counters"}."""
    w, h = fr.size
    pix = _u32(pixels)
    n = pix.shape[0]
    a = abi.CameraRaysArgs()
    rays, index = _guarded(n, 32), _guarded(n, 4)
    a.rays, a.pixel_index, a.pixels = rays.data_ptr() + GUARD * 32, index.data_ptr() + GUARD * 4, pix.data_ptr()
    a.n, a.width, a.height, a.tiling, a.inputs = n, w, h, abi.Tiling(h, 1, 0, h), fr.inputs
    a.flags, a.sample, a.rng_seed, a.rng_frame = abi.RT_CAMERA_JITTER_PHILOX, s, SEED, frame
    rc = lib().rt_camera_rays(C.byref(a), _stream())
    assert rc == 0, (rc, lib().rt_last_error())
    torch.cuda.synchronize()
    assert np.array_equal(_body(index, n, 4, "pixel_index").view(np.uint32).reshape(n), np.asarray(pixels, dtype=np.uint32))
    dense = torch.from_numpy(_body(rays, n, 32, "rays")).cuda()
    b = abi.RadianceArgs()
    out = _guarded(n, 16)
    b.rays, b.stream_ids, b.sum = dense.data_ptr(), pix.data_ptr(), out.data_ptr() + GUARD * 16
    b.n, b.samples_per_ray, b.sample_base, b.max_depth = n, 1, s, fr.depth
    b.flags, b.rng_seed, b.rng_frame = flags, SEED, frame
    b.background_start[:] = list(fr.inputs.background_start)
    b.background_end[:] = list(fr.inputs.background_end)
    counters = torch.zeros(abi.COUNTERS_WORDS, dtype=torch.int64, device="cuda")
    b.counters = counters.data_ptr()
    rc = lib().rt_radiance_rays(fr.ds.handle, C.byref(b), _stream())
    assert rc == 0, (rc, lib().rt_last_error())
    torch.cuda.synchronize()
    total = _body(out, n, 16, "sum").view(F).reshape(n, 4)
    units = total[:, :3].astype(np.float64) * 4096.0
    assert np.all(total[:, 3] == 1) and np.all(units == np.round(units))
    return {"q": units.astype(np.uint64), "counters": counters.cpu().numpy()}


def fused(fr: Frame, pixels, planes: dict, samples=None, count=None, base: int = 1, spp: int = 1, max_samples: int = 16,
          max_history: int = 32, flags: int = DIRECT, rays_per_lane: int = 0, count_tests: int = 0, frame: int = 0) -> dict:
    """One rt_adaptive_samples call: `planes` maps history / moments / accum to their initial (W·H, c) float32 contents;
    returns the planes after the call and "counters", after checking the guards."""
    w, h = fr.size
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
        bufs[o] = _guarded(fr.n, PLANE_BYTES[o])
        body = torch.from_numpy(np.ascontiguousarray(init, dtype=F).view(np.uint8).reshape(-1)).cuda()
        bufs[o][GUARD * PLANE_BYTES[o]:(GUARD + fr.n) * PLANE_BYTES[o]] = body
        setattr(a, o, bufs[o].data_ptr() + GUARD * PLANE_BYTES[o])
    counters = torch.zeros(abi.COUNTERS_WORDS, dtype=torch.int64, device="cuda")
    a.counters, a.count_tests = counters.data_ptr(), count_tests
    a.capacity, a.width, a.height = len(pixels), w, h
    a.samples_per_pixel, a.max_samples, a.sample_base, a.max_depth = spp, max_samples, base, fr.depth
    a.max_history, a.rays_per_lane, a.flags = max_history, rays_per_lane, flags
    a.rng_seed, a.rng_frame = SEED, frame
    a.inputs = fr.inputs
    rc = lib().rt_adaptive_samples(fr.ds.handle, C.byref(a), _stream())
    assert rc == 0, (rc, lib().rt_last_error())
    torch.cuda.synchronize()
    out = {o: _body(bufs[o], fr.n, PLANE_BYTES[o], o).view(F).reshape(fr.n, PLANE_BYTES[o] // 4) for o in planes}
    out["counters"] = counters.cpu().numpy()
    return out


def retrace(fr: Frame, prev_color: np.ndarray, stride: int, offset=(0, 0), k: int = 1, flags: int = DIRECT,
            rays_per_lane: int = 0, count_tests: int = 0, frame: int = 0) -> dict:
    """One rt_temporal_gradient call: prev_color is (W·H, 3) float32; returns the three outputs and "counters", after
    checking the guards."""
    w, h = fr.size
    n = -(-w // stride) * -(-h // stride)
    plane = np.full((fr.n, 4), 7.5, dtype=F)  # (w is never read)
    plane[:, :3] = prev_color
    prev = torch.from_numpy(plane).cuda()
    a = abi.TemporalGradientArgs()
    a.prev_color = prev.data_ptr()
    bufs = {}
    for o, width in OUT_BYTES.items():
        bufs[o] = _guarded(n, width)
        setattr(a, o, bufs[o].data_ptr() + GUARD * width)
    counters = torch.zeros(abi.COUNTERS_WORDS, dtype=torch.int64, device="cuda")
    a.counters, a.count_tests = counters.data_ptr(), count_tests
    a.width, a.height, a.stride, a.offset_x, a.offset_y = w, h, stride, offset[0], offset[1]
    a.samples_per_pixel, a.rays_per_lane, a.flags, a.max_depth = k, rays_per_lane, flags, fr.depth
    a.rng_seed, a.rng_frame = SEED, frame
    a.tiling = abi.Tiling(h, 1, 0, h)
    a.inputs = fr.inputs
    rc = lib().rt_temporal_gradient(fr.ds.handle, C.byref(a), _stream())
    assert rc == 0, (rc, lib().rt_last_error())
    torch.cuda.synchronize()
    out = {}
    for o, width in OUT_BYTES.items():
        raw = _body(bufs[o], n, width, o)
        out[o] = raw.view(np.uint32).reshape(n) if o == "pixel" else raw.view(F).reshape(n, width // 4)
    out["counters"] = counters.cpu().numpy()
    return out


def planes_of(n: int) -> dict:
    """History, moments and accumulation planes with a different value in every pixel."""
    i = np.arange(n, dtype=F)
    hist = np.stack([0.25 + i / 4096.0, 0.5 - i / 8192.0, 0.125 + i / 2048.0, 1.0 + (i % 5)], axis=1).astype(F)
    lum = (0.2126 * hist[:, 0] + 0.7152 * hist[:, 1] + 0.0722 * hist[:, 2]).astype(F)
    return {"history": hist, "moments": np.stack([lum, lum * lum + F(0.01)], axis=1).astype(F),
            "accum": np.stack([hist[:, 0], hist[:, 1], hist[:, 2], np.full(n, 3.0, dtype=F)], axis=1).astype(F)}


def same_planes(a: dict, b: dict, rows=None, what=None) -> None:
    for o in PLANE_BYTES:
        if o in a and o in b:
            assert (a[o] if rows is None else a[o][rows]).tobytes() == (b[o] if rows is None else b[o][rows]).tobytes(), (o, what)


def same_outputs(a: dict, b: dict, what=None) -> None:
    for o in OUT_BYTES:
        assert a[o].tobytes() == b[o].tobytes(), (o, what)


def three_step_merge(fr: Frame, begin: dict, pixels: np.ndarray, k: np.ndarray, base: int, flags: int = DIRECT) -> tuple:
    """The planes after the valid entries' samples base .. base + k_i - 1, each traced by three_step and merged in numpy,
    with the words 0 and 3 of the three-step calls' counters summed."""
    valid = (pixels < fr.n) & (k > 0)
    pix, kk = pixels[valid], k[valid]
    hist, mom = begin["history"][pix].copy(), begin["moments"][pix].copy()
    units = np.zeros((len(pix), 3), dtype=np.uint64)
    rays = paths = 0
    for j in range(int(kk.max())):
        more = np.nonzero(kk > j)[0]
        r = three_step(fr, pix[more], base + j, flags)
        hist[more], mom[more] = merge_history(hist[more], mom[more], r["q"], 32)
        units[more] += r["q"]
        rays += int(r["counters"][0])
        paths += int(r["counters"][3])
    want = {o: v.copy() for o, v in begin.items()}
    want["history"][pix], want["moments"][pix] = hist, mom
    want["accum"][pix] = merge_accum(begin["accum"][pix], units, kk)
    return want, rays, paths


# ---------------------------------------------------------------------------------------------------------------------
# 1. Nothing to sample: the same bits
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["c2_37x21", "c5", "c3_metal", "c3_depth1"])
def test_nothing_to_sample_changes_no_bit(case):
    """No sampled light (c2, c5: the kernel is the flagless one), lights but no diffuse vertex (c3 in metal) and lights
    but no vertex that may connect (c3 at max_depth 1): the flagged fused calls — history with moments, and accum — and
    the flagged gradient call equal the flagless calls, counters included."""
    name = {"c3_metal": "c3", "c3_depth1": "c3"}.get(case, case)
    fr = named(name)
    if case == "c3_metal":
        fr = fr.at(ds=DeviceScene(_metal_c3()))
    if case == "c3_depth1":
        fr = fr.at(depth=1)
    if name != "c3":
        assert lights_of(frame_scene(name))[0] == 0
    orders = (0, LTR) if case in ("c2_37x21", "c3_metal") else (0,)
    begin = planes_of(fr.n)
    pixels = np.arange(fr.n, dtype=np.uint32)
    prev = begin["history"][:, :3]
    results = []
    for order in orders:
        for targets in (("history", "moments"), ("accum",)):
            planes = {o: begin[o] for o in targets}
            plain = fused(fr, pixels, planes, spp=2, flags=order)
            flagged = fused(fr, pixels, planes, spp=2, flags=order | DIRECT)
            same_planes(flagged, plain, what=(order, targets))
            assert np.array_equal(flagged["counters"], plain["counters"])
            assert int(plain["counters"][0]) > 0 and int(plain["counters"][3]) == 2 * fr.n
            assert np.any(plain[targets[0]][:, :3] != begin[targets[0]][:, :3])
        plain = retrace(fr, prev, 1, k=2, flags=order)
        flagged = retrace(fr, prev, 1, k=2, flags=order | DIRECT)
        same_outputs(flagged, plain, order)
        assert np.array_equal(flagged["counters"], plain["counters"]) and int(plain["counters"][3]) == 2 * fr.n
        assert plain["resample"][:, :3].any()
        results.append(plain["resample"].tobytes())
    assert len(set(results)) == len(orders)  # (the fill order matters on these frames)
    if case == "c3_metal":
        fr.ds.close()


# ---------------------------------------------------------------------------------------------------------------------
# 2. Fused equals three steps
# ---------------------------------------------------------------------------------------------------------------------
def listed_entries(n: int, seed: int) -> tuple:
    """About two thirds of the pixels in shuffled order with 0..3 samples each, strangers (indices at or beyond W·H) and
    k = 0 entries of otherwise unlisted pixels among them: (pixels, samples)."""
    rng = np.random.default_rng(seed)
    order = rng.permutation(n).astype(np.uint32)
    cut = (2 * n) // 3
    pixels, rest = order[:cut], order[cut:]
    k = rng.integers(0, 4, cut).astype(np.uint32)
    k[:4] = (3, 0, 1, 2)
    at = len(pixels) // 2
    pixels = np.concatenate([pixels[:at], [n, 0xffffffff, rest[0], n + 7], pixels[at:], [rest[1], 0x7fffffff]]).astype(np.uint32)
    k = np.concatenate([k[:at], [1, 2, 0, 3], k[at:], [0, 1]]).astype(np.uint32)
    return pixels, k


@pytest.mark.parametrize("which", ["c3", "floor"])
def test_fused_equals_three_steps(which):
    """History, moments and accum after the fused flagged call equal the three-step samples merged in numpy, for 0..3
    samples per entry from sample_base 1 and 5; unlisted pixels, the pixels of k = 0 entries and everything an entry at or
    beyond W·H could touch keep their bits; counters[0] and [3] are the three-step calls' totals; and the flag matters: some
    listed pixel differs from the flagless fused call, which traces fewer rays."""
    fr = named("c3") if which == "c3" else floor_frame()
    begin = planes_of(fr.n)
    pixels, k = listed_entries(fr.n, 11 if which == "c3" else 12)
    assert np.sum(k == 0) > 4 and np.sum(k == 3) > 4 and len(np.unique(pixels)) == len(pixels)
    listed = np.zeros(fr.n, dtype=bool)
    listed[pixels[(pixels < fr.n) & (k > 0)]] = True
    for base in (1, 5):
        want, rays, paths = three_step_merge(fr, begin, pixels, k, base)
        got = fused(fr, pixels, begin, samples=k, base=base)
        wrong = np.nonzero(np.any(got["accum"] != want["accum"], axis=1))[0]
        print(f"{which} base {base}: rays {int(got['counters'][0])} (three steps {rays}), paths {paths}, differing pixels {len(wrong)}")
        assert len(wrong) == 0, (len(wrong), wrong[:8], got["accum"][wrong[:4]], want["accum"][wrong[:4]])
        same_planes(got, want, what=base)
        same_planes(got, begin, ~listed, what=base)
        assert np.any(got["accum"][listed, :3] != begin["accum"][listed, :3])
        assert int(got["counters"][0]) == rays and int(got["counters"][3]) == paths == int(k[pixels < fr.n].sum())
        plain = fused(fr, pixels, begin, samples=k, base=base, flags=0)
        assert np.any(plain["accum"][listed] != got["accum"][listed]) and np.any(plain["history"][listed] != got["history"][listed])
        assert int(got["counters"][0]) > int(plain["counters"][0]) and int(plain["counters"][3]) == paths
    # each target alone, and history without moments
    for only in (("accum",), ("history",), ("history", "moments")):
        same_planes(fused(fr, pixels, {o: begin[o] for o in only}, samples=k, base=5), want, what=only)


# ---------------------------------------------------------------------------------------------------------------------
# 3. Composition
# ---------------------------------------------------------------------------------------------------------------------
def test_composition():
    """Three samples in one call equal three chained one-sample calls with sample_base stepping; max_samples caps an
    entry; max_depth = 0 merges zeros and traces nothing."""
    fr = named("c3")
    begin = planes_of(fr.n)
    pixels = np.arange(fr.n, dtype=np.uint32)
    whole = fused(fr, pixels, begin, spp=3, base=2)
    chained, rays = begin, 0
    for j in range(3):
        chained = fused(fr, pixels, {o: chained[o] for o in PLANE_BYTES}, spp=1, base=2 + j)
        rays += int(chained["counters"][0])
    same_planes(whole, chained)
    assert int(whole["counters"][0]) == rays and int(whole["counters"][3]) == 3 * fr.n
    assert np.all(whole["accum"][:, 3] == begin["accum"][:, 3] + 3)
    same_planes(fused(fr, pixels, begin, samples=np.full(fr.n, 9, dtype=np.uint32), max_samples=3, base=2), whole)
    dark = fused(fr.at(depth=0), pixels, begin, spp=3, base=2)
    assert int(dark["counters"][0]) == 0 and int(dark["counters"][3]) == 3 * fr.n
    assert np.array_equal(dark["accum"][:, :3], begin["accum"][:, :3]) and np.all(dark["accum"][:, 3] == begin["accum"][:, 3] + 3)
    hw, mw = begin["history"], begin["moments"]
    for _ in range(3):
        hw, mw = merge_history(hw, mw, np.zeros((fr.n, 3), dtype=np.uint32), 32)
    assert dark["history"].tobytes() == hw.tobytes() and dark["moments"].tobytes() == mw.tobytes()
    black = retrace(fr.at(depth=0), begin["history"][:, :3], 3, (1, 2), k=3)
    assert int(black["counters"][0]) == 0 and not black["resample"][:, :3].any()


# ---------------------------------------------------------------------------------------------------------------------
# 4. Gradient
# ---------------------------------------------------------------------------------------------------------------------
def frame_colour(fr: Frame, k: int) -> np.ndarray:
    """The k-spp radiance plane of a flagged frame by the three-step path: (W·H, 3) float32."""
    pixels = np.arange(fr.n, dtype=np.uint32)
    return mean_color([three_step(fr, pixels, s)["q"] for s in range(k)])


LAYOUTS = ((1, (0, 0)), (3, (0, 0)), (3, (2, 1)), (8, (0, 0)))


@pytest.mark.parametrize("which,k", [("c3", 1), ("c3", 3), ("floor", 2)])
def test_gradient_of_an_unedited_flagged_frame_is_zero(which, k):
    """prev_color by the three-step flagged path: every stratum has δ = 0 exactly, resample has prev_color's bits at the
    stratum's pixel, and the pixel plane is right, at stride 1, 3 (two offsets) and 8.  The flagless call on the same
    plane finds δ > 0 (c3)."""
    fr = named("c3") if which == "c3" else floor_frame()
    w, h = fr.size
    c_old = frame_colour(fr, k)
    assert c_old.any()
    for stride, offset in LAYOUTS:
        want = gradient_reference(c_old, c_old, w, h, stride, offset)
        got = retrace(fr, c_old, stride, offset, k=k)
        assert not got["gradient"][:, 0].any(), (stride, offset, np.nonzero(got["gradient"][:, 0])[0][:8])
        assert got["resample"][:, :3].tobytes() == c_old[strata_pixels(w, h, stride, offset)].tobytes()
        same_outputs(got, want, (stride, offset))
        assert int(got["counters"][3]) == k * len(want["pixel"])
    if which == "c3":
        plain = retrace(fr, c_old, 1, k=k, flags=0)
        changed = float((plain["gradient"][:, 0] > 0).mean())
        print(f"c3 k {k}: strata of a flagged frame the flagless call finds changed: {changed:.3f}")
        assert changed > 0


def test_gradient_after_a_lamp_edit():
    """The lamp's intensity changes (rt_scene_update_materials): resample equals the three-step result in the edited
    scene, δ > 0 in some stratum and δ = 0 in every stratum whose three-step result is unchanged."""
    base = named("c3")
    scene = scenes.Scene.from_bytes(frame_scene("c3").hittables_bytes(), frame_scene("c3").materials_bytes())
    ds = DeviceScene(scene)
    fr = base.at(ds=ds)
    w, h = fr.size
    k = 2
    c_old = frame_colour(fr, k)
    assert c_old.tobytes() == frame_colour(base, k).tobytes()
    lamps = [m for m in scene.materials if m.type == abi.RT_DIFFUSELIGHT]
    assert len(lamps) == 1
    lamps[0].light_intensity = lamps[0].light_intensity + 5
    ds.update_materials(scene.materials)
    c_new = frame_colour(fr, k)
    for stride, offset in LAYOUTS:
        want = gradient_reference(c_old, c_new, w, h, stride, offset)
        got = retrace(fr, c_old, stride, offset, k=k)
        same_outputs(got, want, (stride, offset))
        pix = strata_pixels(w, h, stride, offset)
        unchanged = np.all(c_new[pix] == c_old[pix], axis=1)
        assert np.any(got["gradient"][:, 0] > 0) and not got["gradient"][unchanged, 0].any()
        print(f"stride {stride} offset {offset}: strata {len(pix)}, unchanged {int(unchanged.sum())}")
    assert np.all(c_new == c_old, axis=1).sum() < fr.n  # (the edit shows)
    ds.close()


# ---------------------------------------------------------------------------------------------------------------------
# 5. Schedule
# ---------------------------------------------------------------------------------------------------------------------
COUNTS = {1: (1, 1), 63: (9, 7), 65: (13, 5), 64 * 16 + 1: (41, 25)}  # items: a (w, h) with w · h strata at stride 1
LANES = (1, 3, 16)
TUNINGS = ((abi.RT_TUNE_REGEN_THRESHOLD, 1), (abi.RT_TUNE_REGEN_THRESHOLD, 64), (abi.RT_TUNE_LEAF_BREAK, 0),
           (abi.RT_TUNE_LEAF_BREAK, 64))


def test_schedule_independence_of_the_fused_call():
    """rays_per_lane 1, 3 and 16 at 1, 63, 65 and 1025 entries of a 41 x 25 frame; a device count below the capacity; the
    counting build; two settings each of the regeneration threshold and the leaf-break rule: the same bytes."""
    fr = named("c3").at(size=(41, 25))
    assert fr.n == 64 * 16 + 1
    begin = planes_of(fr.n)
    order = np.random.default_rng(5).permutation(fr.n).astype(np.uint32)
    samples = (1 + (order * 7 + order // 5) % 3).astype(np.uint32)  # 1..3 paths, mixed within every wave
    for m in COUNTS:
        whole = fused(fr, order[:m], begin, samples=samples[:m], base=0)
        assert int(whole["counters"][3]) == int(samples[:m].sum())
        for rpl in LANES:
            got = fused(fr, order[:m], begin, samples=samples[:m], base=0, rays_per_lane=rpl)
            same_planes(got, whole, what=(m, rpl))
            assert np.array_equal(got["counters"][[0, 3]], whole["counters"][[0, 3]])
        # the same entries as the head of the whole list, counted on the device
        same_planes(fused(fr, order, begin, samples=samples, base=0, count=[m, 0], rays_per_lane=3), whole, what=("count", m))
    counted = fused(fr, order, begin, samples=samples, base=0, count_tests=1)
    same_planes(counted, whole)
    assert int(counted["counters"][0]) == int(whole["counters"][0]) and int(counted["counters"][1]) > 0
    for key, v in TUNINGS:
        prev = lib().rt_set_tuning(key, v)
        try:
            same_planes(fused(fr, order, begin, samples=samples, base=0, rays_per_lane=3), whole, what=(key, v))
        finally:
            lib().rt_set_tuning(key, prev)


def test_schedule_independence_of_the_gradient_call():
    """The same for rt_temporal_gradient at stride 1 on frames of 1, 63, 65 and 1025 strata, three samples each."""
    for m, size in COUNTS.items():
        fr = named("c3").at(size=size)
        prev = planes_of(fr.n)["history"][:, :3]
        whole = retrace(fr, prev, 1, k=3)
        assert len(whole["pixel"]) == m and int(whole["counters"][3]) == 3 * m
        for rpl in LANES:
            got = retrace(fr, prev, 1, k=3, rays_per_lane=rpl)
            same_outputs(got, whole, (m, rpl))
            assert np.array_equal(got["counters"][[0, 3]], whole["counters"][[0, 3]])
    counted = retrace(fr, prev, 1, k=3, count_tests=1)
    same_outputs(counted, whole)
    assert int(counted["counters"][0]) == int(whole["counters"][0]) and int(counted["counters"][1]) > 0
    for key, v in TUNINGS:
        old = lib().rt_set_tuning(key, v)
        try:
            same_outputs(retrace(fr, prev, 1, k=3, rays_per_lane=3), whole, (key, v))
        finally:
            lib().rt_set_tuning(key, old)


# ---------------------------------------------------------------------------------------------------------------------
# 6. 32-bit references
# ---------------------------------------------------------------------------------------------------------------------
def test_wide_references_and_the_light_list():
    """The builds for scenes with 32-bit BVH references: the flagged fused call equals three steps and the flagged re-trace
    of that frame is all zero; an edited copy (rt_scene_edit) still has the lamp; after rt_scene_update_materials turns
    the lamp off the flagged call is the flagless one."""
    plain_scene, lamp_scene = _wide_with_rect(False), _wide_with_rect(True)
    assert lights_of(lamp_scene)[0] == 1 and lights_of(plain_scene)[0] == 0
    ds = DeviceScene(lamp_scene)
    assert ds.info().num_primitives >= 8192
    fr = Frame(ds, frame_inputs("wide_near"), (37, 21), 6)
    begin = planes_of(fr.n)
    pixels = np.arange(fr.n, dtype=np.uint32)
    k = (1 + pixels % 2).astype(np.uint32)
    want, rays, paths = three_step_merge(fr, begin, pixels, k, 1)
    got = fused(fr, pixels, begin, samples=k)
    same_planes(got, want)
    assert int(got["counters"][0]) == rays and int(got["counters"][3]) == paths
    plain = fused(fr, pixels, begin, samples=k, flags=0)
    assert np.any(plain["accum"] != got["accum"]) and int(got["counters"][0]) > int(plain["counters"][0])
    c_old = frame_colour(fr, 2)
    for stride, offset in ((1, (0, 0)), (3, (2, 1))):
        zero = retrace(fr, c_old, stride, offset, k=2)
        same_outputs(zero, gradient_reference(c_old, c_old, 37, 21, stride, offset), (stride, offset))
        assert not zero["gradient"][:, 0].any()
    edited = ds.edited(lamp_scene.hittables)
    same_planes(fused(fr.at(ds=edited), pixels, begin, samples=k), want, what="edited")
    edited.close()
    ds.update_materials(plain_scene.materials)
    off = fused(fr, pixels, begin, samples=k)
    plain_off = fused(fr, pixels, begin, samples=k, flags=0)
    same_planes(off, plain_off, what="lamp off")
    assert np.array_equal(off["counters"], plain_off["counters"]) and np.any(off["accum"] != got["accum"])
    ds.close()


# ---------------------------------------------------------------------------------------------------------------------
# 7. Python
# ---------------------------------------------------------------------------------------------------------------------
def test_device_scene_wrappers_are_the_direct_calls():
    fr = named("c3")
    w, h = fr.size
    begin = planes_of(fr.n)
    pixels, k = listed_entries(fr.n, 21)
    want = fused(fr, pixels, begin, samples=k, base=2, flags=DIRECT | LTR)
    dev = {o: torch.from_numpy(begin[o].reshape(h, w, -1).copy()).cuda() for o in PLANE_BYTES}
    fr.ds.adaptive_samples(_u32(pixels), fr.inputs, w, h, fr.depth, samples=_u32(k), sample_base=2, seed=SEED,
                           left_to_right=True, direct_light=True, **dev)
    torch.cuda.synchronize()
    same_planes({o: t.cpu().numpy().reshape(fr.n, -1) for o, t in dev.items()}, want)
    c_old = frame_colour(fr, 2)
    direct = retrace(fr, c_old, 3, (2, 1), k=2)
    prev = torch.from_numpy(np.concatenate([c_old, np.ones((fr.n, 1), dtype=F)], axis=1)).cuda()
    sw, sh = -(-w // 3), -(-h // 3)
    resample = torch.zeros((sh, sw, 4), dtype=torch.float32, device="cuda")
    pixel = torch.zeros((sh, sw), dtype=torch.int32, device="cuda")
    grad = fr.ds.temporal_gradient(prev, fr.inputs, w, h, fr.depth, stride=3, offset=(2, 1), samples_per_pixel=2, seed=SEED,
                                   resample=resample, pixel=pixel, direct_light=True)
    torch.cuda.synchronize()
    assert grad.cpu().numpy().tobytes() == direct["gradient"].tobytes() and not direct["gradient"][:, 0].any()
    assert resample.cpu().numpy().tobytes() == direct["resample"].tobytes()
    assert pixel.cpu().numpy().view(np.uint32).tobytes() == direct["pixel"].tobytes()
    # without the keyword the wrapper is the flagless call
    plain = fr.ds.temporal_gradient(prev, fr.inputs, w, h, fr.depth, stride=3, offset=(2, 1), samples_per_pixel=2, seed=SEED)
    torch.cuda.synchronize()
    assert plain.cpu().numpy().tobytes() == retrace(fr, c_old, 3, (2, 1), k=2, flags=0)["gradient"].tobytes()


def test_renderer_render_direct_and_what_follows():
    """Renderer.render_direct at 1, 2 and 3 spp: the radiance plane is the three-step sums divided in numpy float32; the
    frame counter advances; temporal_gradient() on the unedited scene returns an all-zero δ plane and leaves every history
    length's bits alone; adaptive() continues the frame with the flag, as the explicit flagged call does."""
    fr = named("c3")
    w, h = fr.size
    pixels = np.arange(fr.n, dtype=np.uint32)
    r = Renderer(w, h, rng="philox")
    r.render_init(SEED)
    for frame, spp in enumerate((1, 2, 3)):
        assert r.frame == frame
        r.render_direct(fr.ds, fr.inputs, spp=spp, depth=fr.depth)
        torch.cuda.synchronize()
        units = sum(three_step(fr, pixels, s, frame=frame)["q"] for s in range(spp))
        want = ((units.astype(F) * F(1.0 / 4096.0)).astype(F) / F(spp)).astype(F)
        got = r.radiance.cpu().numpy().reshape(fr.n, 4)
        assert got[:, :3].tobytes() == want.tobytes(), spp
        assert np.all(got[:, 3] == 1) and r.frame == frame + 1
        assert r._radiance_frame[2:] == (frame, spp, abi.RT_FLAG_RNG_PHILOX | DIRECT)
    flagless = r.render_direct(fr.ds, fr.inputs, spp=1, depth=fr.depth, direct_light=False).cpu().numpy().reshape(fr.n, 4)
    assert flagless[:, :3].tobytes() == (three_step(fr, pixels, 0, flags=0, frame=3)["q"].astype(F) * F(1.0 / 4096.0)).astype(F).tobytes()
    # the chain: frame -> temporal -> gradient -> adaptive, on one estimator
    r.render_direct(fr.ds, fr.inputs, spp=2, depth=fr.depth)
    frame = r.frame - 1
    r.gbuffer(fr.ds, fr.inputs)
    r.temporal(moments=True)
    torch.cuda.synchronize()
    hist0, mom0 = r.history.cpu().numpy().copy(), r.moments.cpu().numpy().copy()
    for _ in range(2):  # (two positions of the pixel in its stratum)
        grad = r.temporal_gradient(fr.ds, fr.depth, stride=3)
        torch.cuda.synchronize()
        assert not grad.cpu().numpy()[..., 0].any()
        assert r.history.cpu().numpy().tobytes() == hist0.tobytes()
    params = dict(tau=0.1, lum_floor=0.01, min_history=3, max_samples=2)
    count = r.adaptive(fr.ds, fr.inputs, fr.depth, sample_base=2, **params)
    torch.cuda.synchronize()
    listed = int(count.cpu().numpy()[0])
    assert listed > fr.n // 2
    got_h, got_m = r.history.cpu().numpy().copy(), r.moments.cpu().numpy().copy()
    results = {}
    for flag in (True, False):
        hist = torch.from_numpy(hist0.copy()).cuda()
        mom = torch.from_numpy(mom0.copy()).cuda()
        fr.ds.adaptive_samples(r.adaptive_pixels, fr.inputs, w, h, fr.depth, samples=r.adaptive_samples, count=r.adaptive_count,
                               history=hist, moments=mom, max_samples=2, sample_base=2, seed=SEED, frame=frame,
                               direct_light=flag)
        torch.cuda.synchronize()
        results[flag] = (hist.cpu().numpy().tobytes(), mom.cpu().numpy().tobytes())
    assert (got_h.tobytes(), got_m.tobytes()) == results[True] != results[False]
    assert got_h.tobytes() != hist0.tobytes()
    # the keyword overrides the recorded frame's bit
    r.history.copy_(torch.from_numpy(hist0).cuda())
    r.moments.copy_(torch.from_numpy(mom0).cuda())
    r.adaptive(fr.ds, fr.inputs, fr.depth, sample_base=2, direct_light=False, **params)
    torch.cuda.synchronize()
    assert (r.history.cpu().numpy().tobytes(), r.moments.cpu().numpy().tobytes()) == results[False]
