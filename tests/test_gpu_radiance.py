"""rt_radiance_rays and rt_camera_rays on the GPU.

Frames, scenes and the reference are those of tests/test_radiance_host.py: sample s of a pixel is the difference of two
oracle Philox frames in 2^-12 units, and the host test has shown that on these frames the comparison is decidable on
every ray.  Every call goes to the C entry points directly, with the outputs filled with 0x5a and 16 guard elements
before and after each, checked after the call.  Everything is compared bit for bit: the kernels' samples and ray counts
with the oracle's, a many-sample call with the fixed-point sum of one-sample calls, listed pixels with the dense frame,
rt_camera_rays' centre rays (through rt_query_rays) with rt_gbuffer, and the outputs across schedules."""
from __future__ import annotations

import ctypes as C

import numpy as np
import pytest
import torch

from cudaraytracer_amd import abi, scenes
from cudaraytracer_amd._lib import lib
from cudaraytracer_amd.renderer import DeviceScene, band_rows_of, camera_rays

from test_denoise_host import FLT_MAX
from test_radiance_host import FRAMES, SAMPLES, SEED, frame_inputs, frame_scene, sample_reference

pytestmark = pytest.mark.gpu

F = np.float32
GUARD = 16   # guard elements before and after every output
FILL = 0x5a  # byte the outputs and their guards are filled with

_device_scenes = {}


def device_scene(name: str) -> DeviceScene:
    if name not in _device_scenes:
        _device_scenes[name] = DeviceScene(frame_scene(name))
    return _device_scenes[name]


def _stream() -> C.c_void_p:
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _guarded(n: int, width: int) -> torch.Tensor:
    return torch.full(((n + 2 * GUARD) * width,), FILL, dtype=torch.uint8, device="cuda")


def _body(buf: torch.Tensor, n: int, width: int, what: str) -> np.ndarray:
    raw = buf.cpu().numpy().reshape(n + 2 * GUARD, width)
    assert np.all(raw[:GUARD] == FILL) and np.all(raw[n + GUARD:] == FILL), what
    return raw[GUARD:n + GUARD].copy()


def camera(name: str, jitter="philox", sample: int = 0, pixels: torch.Tensor | None = None,
           tiling: abi.Tiling | None = None, outputs=("rays", "pixel_index")) -> tuple:
    """One direct rt_camera_rays call for a frame: (rays tensor (n, 2, 4), pixel_index tensor (n,) int32), after checking
    the guards of both outputs."""
    w, h = FRAMES[name][2]
    t = tiling if tiling is not None else abi.Tiling(h, 1, 0, h)
    n = pixels.shape[0] if pixels is not None else t.local_rows * w
    a = abi.CameraRaysArgs()
    rays, index = _guarded(n, 32), _guarded(n, 4)
    a.rays = rays.data_ptr() + GUARD * 32
    if "pixel_index" in outputs:
        a.pixel_index = index.data_ptr() + GUARD * 4
    if pixels is not None:
        a.pixels = pixels.data_ptr()
    a.n, a.width, a.height, a.tiling, a.inputs = n, w, h, t, frame_inputs(name)
    if jitter == "philox":
        a.flags, a.sample, a.rng_seed, a.rng_frame = abi.RT_CAMERA_JITTER_PHILOX, sample, SEED, 0
    else:
        a.xi1, a.xi2 = jitter
    rc = lib().rt_camera_rays(C.byref(a), _stream())
    assert rc == 0, (rc, lib().rt_last_error())
    torch.cuda.synchronize()
    r = torch.from_numpy(_body(rays, n, 32, "rays").view(F).reshape(n, 2, 4)).cuda()
    raw = _body(index, n, 4, "pixel_index")
    i = torch.from_numpy(raw.view(np.int32).reshape(n)).cuda() if "pixel_index" in outputs else None
    if i is None:
        assert np.all(raw == FILL)
    return r, i


def radiance(ds: DeviceScene, name: str, rays: torch.Tensor, n: int, ids: torch.Tensor | None = None, base: int = 0,
             samples: int = 1, depth: int | None = None, flags: int = 0, rays_per_lane: int = 0,
             count_tests: int | None = 0, stream_base: int = 0, outputs=("sum", "mean")) -> dict:
    """One direct rt_radiance_rays call on the first n rays with the frame's sky and depth: {"sum", "mean": (n, 4)
    float32, "q": sum.rgb in 2^-12 units as uint32, "counters"}, after checking the guards."""
    inp = frame_inputs(name)
    a = abi.RadianceArgs()
    a.rays = rays.data_ptr()
    bufs = {}
    for o in outputs:
        bufs[o] = _guarded(n, 16)
        setattr(a, o, bufs[o].data_ptr() + GUARD * 16)
    if ids is not None:
        a.stream_ids = ids.data_ptr()
    a.n, a.rays_per_lane, a.samples_per_ray, a.sample_base = n, rays_per_lane, samples, base
    a.max_depth = FRAMES[name][3] if depth is None else depth
    a.flags, a.stream_base, a.rng_seed, a.rng_frame = flags, stream_base, SEED, 0
    a.background_start[:] = list(inp.background_start)
    a.background_end[:] = list(inp.background_end)
    counters = None
    if count_tests is not None:
        counters = torch.zeros(abi.COUNTERS_WORDS, dtype=torch.int64, device="cuda")
        a.counters, a.count_tests = counters.data_ptr(), count_tests
    rc = lib().rt_radiance_rays(ds.handle, C.byref(a), _stream())
    assert rc == 0, (rc, lib().rt_last_error())
    torch.cuda.synchronize()
    out = {o: _body(bufs[o], n, 16, o).view(F).reshape(n, 4) for o in outputs}
    if "sum" in out:
        assert np.all(out["sum"][:, 3] == F(samples))
        units = out["sum"][:, :3].astype(np.float64) * 4096.0
        assert np.all(units == np.round(units))
        out["q"] = units.astype(np.uint64)  # (exact below 2^24 units; a saturated sum reads 2^32)
    if "mean" in out:
        assert np.all(out["mean"][:, 3] == F(1.0))
    if counters is not None:
        out["counters"] = counters.cpu().numpy()
    return out


def same_bits(a: dict, b: dict, n: int | None = None) -> None:
    for o in ("sum", "mean"):
        if o in a and o in b:
            assert a[o][:n].tobytes() == b[o][:n].tobytes(), o


def sky_units(rays: np.ndarray, inp: abi.InputStruct) -> np.ndarray:
    """color() of rays that hit nothing (Kernel.cu:41-44) in 2^-12 units, with the kernel's float32 operations."""
    d = rays[:, 1, :3].astype(F)
    length = np.sqrt((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2], dtype=F)
    t = F(0.5) * (d[:, 1] / length + F(1.0))
    b0, b1 = np.array(list(inp.background_start), dtype=F), np.array(list(inp.background_end), dtype=F)
    c = (F(1.0) - t)[:, None] * b0[None, :] + t[:, None] * b1[None, :]
    return (c * F(4096.0) + F(0.5)).astype(np.uint32)


# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(FRAMES))
def test_oracle_parity(name):
    """Every ray, bit for bit: the Philox camera ray of sample s, traced with its pixel index as stream id and
    sample_base = s, returns the sample the oracle's Philox frame adds for that pixel, and the launch traces the rays
    the oracle counts for that sample.  (c2 37x21: under both Random() fill orders.)"""
    ds = device_scene(name)
    w, h = FRAMES[name][2]
    n = w * h
    orders = ((0, 1), (abi.RT_FLAG_RIUS_LEFT_TO_RIGHT, 0)) if name == "c2_37x21" else ((0, 1),)
    for s in range(SAMPLES):
        rays, index = camera(name, "philox", s)
        assert np.array_equal(index.cpu().numpy(), np.arange(n, dtype=np.int32))
        for flags, rius in orders:
            want, want_rays = sample_reference(name, s, rius_order=rius)
            got = radiance(ds, name, rays, n, ids=index, base=s, flags=flags)
            wrong = np.nonzero(np.any(got["q"] != want, axis=1))[0]
            print(f"{name} sample {s} flags {flags}: rays {int(got['counters'][0])} (oracle {want_rays}), differing rays {len(wrong)}")
            assert len(wrong) == 0, (len(wrong), wrong[:8], got["q"][wrong[:4]], want[wrong[:4]])
            assert int(got["counters"][0]) == want_rays and int(got["counters"][3]) == n
            assert got["mean"][:, :3].tobytes() == got["sum"][:, :3].tobytes()  # (one sample: x / 1)
            # without ids: stream_base + i is the same stream for a dense frame
            same_bits(radiance(ds, name, rays, n, base=s, flags=flags, count_tests=None), got)


def test_composition():
    """One call with 3 samples from base 1 is the saturating sum of three one-sample calls; mean is sum.rgb / 3 by the
    render's (IEEE) division; its counters are the three calls' together."""
    name = "c2_40x24"
    ds = device_scene(name)
    n = 40 * 24
    rays, index = camera(name, "philox", 1)
    whole = radiance(ds, name, rays, n, ids=index, base=1, samples=3, count_tests=1)
    parts = [radiance(ds, name, rays, n, ids=index, base=1 + k, count_tests=1) for k in range(3)]
    total = np.minimum(sum(p["q"] for p in parts), np.uint64(0xffffffff))
    assert np.array_equal(whole["q"], total)
    assert len({p["q"].tobytes() for p in parts}) == 3  # (three different samples)
    assert whole["mean"][:, :3].tobytes() == (whole["sum"][:, :3] / F(3.0)).astype(F).tobytes()
    for word in (0, 3):  # rays and paths: sums over the batch's rays, whatever the schedule
        assert int(whole["counters"][word]) == sum(int(p["counters"][word]) for p in parts), word
    assert int(whole["counters"][3]) == 3 * n


def test_sparse_equals_dense():
    """Listed pixels (shuffled, with duplicates) and the bands of a 2-rank tiling give the dense frame's rays and
    values at those pixels."""
    name = "c2_37x21"
    ds = device_scene(name)
    w, h = FRAMES[name][2]
    rays, index = camera(name, "philox", 1)
    dense = radiance(ds, name, rays, w * h, ids=index, base=1)
    dense_rays = rays.cpu().numpy()
    pick = np.random.default_rng(5).integers(0, w * h, 100).astype(np.int32)
    assert len(np.unique(pick)) < 100 and np.any(np.diff(pick) < 0)
    p_rays, p_index = camera(name, "philox", 1, pixels=torch.from_numpy(pick).cuda())
    assert np.array_equal(p_index.cpu().numpy(), pick)
    assert p_rays.cpu().numpy().tobytes() == dense_rays[pick].tobytes()
    got = radiance(ds, name, p_rays, 100, ids=p_index, base=1)
    assert got["sum"].tobytes() == dense["sum"][pick].tobytes() and got["mean"].tobytes() == dense["mean"][pick].tobytes()
    seen = []
    for rank in (0, 1):
        rows = band_rows_of(h, 8, 2, rank)
        t = abi.Tiling(8, 2, rank, len(rows))
        b_rays, b_index = camera(name, "philox", 1, tiling=t)
        idx = b_index.cpu().numpy()
        assert np.array_equal(idx, (np.array(rows)[:, None] * w + np.arange(w)[None, :]).reshape(-1))
        assert b_rays.cpu().numpy().tobytes() == dense_rays[idx].tobytes()
        got = radiance(ds, name, b_rays, len(idx), ids=b_index, base=1)
        assert got["sum"].tobytes() == dense["sum"][idx].tobytes()
        seen.append(idx)
    assert np.array_equal(np.sort(np.concatenate(seen)), np.arange(w * h))


def _gbuffer(ds: DeviceScene, name: str, t: abi.Tiling) -> dict:
    w, h = FRAMES[name][2]
    n = t.local_rows * w
    a = abi.GBufferArgs()
    bufs = {"normal_depth": _guarded(n, 16), "albedo": _guarded(n, 16), "prim_id": _guarded(n, 4)}
    for o, b in bufs.items():
        setattr(a, o, b.data_ptr() + GUARD * (4 if o == "prim_id" else 16))
    a.width, a.height, a.tiling, a.inputs = w, h, t, frame_inputs(name)
    assert lib().rt_gbuffer(ds.handle, C.byref(a), _stream()) == 0, lib().rt_last_error()
    torch.cuda.synchronize()
    return {o: _body(b, n, 4 if o == "prim_id" else 16, o) for o, b in bufs.items()}


@pytest.mark.parametrize("name,tiling", [("c2_40x24", None), ("c2_37x21", (8, 2, 0)), ("c2_37x21", (8, 2, 1))])
def test_centre_rays_are_the_gbuffers(name, tiling):
    """rt_query_rays on rt_camera_rays' (0.5, 0.5) rays equals rt_gbuffer's planes bit for bit on every pixel, with no
    undecidable allowance: normal_depth and prim_id everywhere, albedo on every hit (on a miss rt_gbuffer stores the
    sky's colour and rt_query_rays, which has no camera, zeros)."""
    ds = device_scene(name)
    w, h = FRAMES[name][2]
    t = abi.Tiling(h, 1, 0, h) if tiling is None else abi.Tiling(*tiling, len(band_rows_of(h, tiling[0], tiling[1], tiling[2])))
    n = t.local_rows * w
    rays, _ = camera(name, (0.5, 0.5), tiling=t, outputs=("rays",))
    r = rays.cpu().numpy()
    assert np.all(r[:, 0, 3] == F(0.001)) and np.all(r[:, 1, 3] == F(FLT_MAX))
    a = abi.QueryArgs()
    bufs = {"normal_depth": _guarded(n, 16), "albedo": _guarded(n, 16), "prim_id": _guarded(n, 4)}
    for o, b in bufs.items():
        setattr(a, o, b.data_ptr() + GUARD * (4 if o == "prim_id" else 16))
    a.rays, a.n = rays.data_ptr(), n
    assert lib().rt_query_rays(ds.handle, C.byref(a), _stream()) == 0, lib().rt_last_error()
    torch.cuda.synchronize()
    got = {o: _body(b, n, 4 if o == "prim_id" else 16, o) for o, b in bufs.items()}
    want = _gbuffer(ds, name, t)
    assert got["prim_id"].tobytes() == want["prim_id"].tobytes()
    assert got["normal_depth"].tobytes() == want["normal_depth"].tobytes()
    hit = got["prim_id"].view(np.int32).reshape(n) >= 0
    assert 0.2 < hit.mean() <= 1.0
    assert got["albedo"][hit].tobytes() == want["albedo"][hit].tobytes()
    assert not got["albedo"][~hit].any()


def test_schedule_independence():
    """rays_per_lane, batch sizes around a wave and around a lane's 16 rays, two non-default tunings and a repeated
    call: the same bits."""
    name = "c2_37x21"
    ds = device_scene(name)
    rays, index = camera(name, "philox", 0)
    n = 64 * 16 + 1
    reps = -(-n // rays.shape[0])
    rays, index = rays.repeat(reps, 1, 1)[:n].contiguous(), index.repeat(reps)[:n].contiguous()
    whole = radiance(ds, name, rays, n, ids=index, samples=2)
    assert whole["sum"][:248].tobytes() == whole["sum"][777:n].tobytes()  # (the appended rays are the first 248 again)
    same_bits(radiance(ds, name, rays, n, ids=index, samples=2), whole)
    for rpl in (0, 1, 3, 16):
        same_bits(radiance(ds, name, rays, n, ids=index, samples=2, rays_per_lane=rpl), whole)
    for m in (1, 63, 64, 65, n):
        for rpl in (0, 16):
            same_bits(radiance(ds, name, rays, m, ids=index, samples=2, rays_per_lane=rpl), whole, m)
    for key, values in ((abi.RT_TUNE_REGEN_THRESHOLD, (1, 64)), (abi.RT_TUNE_LEAF_BREAK, (0, 64))):
        for v in values:
            prev = lib().rt_set_tuning(key, v)
            try:
                same_bits(radiance(ds, name, rays, n, ids=index, samples=2, rays_per_lane=3), whole)
            finally:
                lib().rt_set_tuning(key, prev)
    # each output alone, and the counting build
    for only in ("sum", "mean"):
        same_bits(radiance(ds, name, rays, n, ids=index, samples=2, outputs=(only,)), whole)
    counted = radiance(ds, name, rays, n, ids=index, samples=2, count_tests=1)
    same_bits(counted, whole)
    assert int(counted["counters"][0]) == int(whole["counters"][0]) and int(counted["counters"][1]) > 0
    # ids are streams: base + i without a list, and another stream gives another sample
    plain = radiance(ds, name, rays, 777, base=0, samples=2, stream_base=0)
    same_bits(plain, whole, 777)
    other = radiance(ds, name, rays, 777, base=0, samples=2, stream_base=1000)
    assert other["sum"].tobytes() != plain["sum"].tobytes()


def test_edges():
    """Empty and all-inactive scenes give the sky; max_depth = 0 gives zeros and traces nothing; n = 0 is accepted; an
    out-of-frame pixel index gives the empty-range ray, which nothing occludes."""
    name = "c2_37x21"
    rays, index = camera(name, "philox", 0)
    n = 777
    want = sky_units(rays.cpu().numpy(), frame_inputs(name))
    three = scenes.builtin(scenes.SCENE_THREE_SPHERES)
    empty = scenes.Scene((abi.HittableDesc * 0)(), three.materials, [])
    for h in three.hittables:
        h.is_active = 0
    for s in (empty, three):
        ds = DeviceScene(s)
        got = radiance(ds, name, rays, n, ids=index, samples=1)
        assert np.array_equal(got["q"], want)
        assert int(got["counters"][0]) == n and int(got["counters"][3]) == n
        two = radiance(ds, name, rays, n, ids=index, samples=2)
        assert np.array_equal(two["q"], 2 * want.astype(np.uint64))
        ds.close()
    ds = device_scene(name)
    got = radiance(ds, name, rays, n, ids=index, samples=3, depth=0)
    assert not got["sum"][:, :3].any() and not got["mean"][:, :3].any()
    assert int(got["counters"][0]) == 0 and int(got["counters"][3]) == 3 * n
    # depth 1 on a frame that sees sky: the sky where the camera ray misses, 0 where it hits (no emitters there)
    far_rays, far_index = camera("wide_far", "philox", 0)
    one = radiance(device_scene("wide_far"), "wide_far", far_rays, n, ids=far_index, depth=1)
    sky = np.all(one["q"] == sky_units(far_rays.cpu().numpy(), frame_inputs("wide_far")), axis=1)
    assert int(one["counters"][0]) == n and 0.25 * n < sky.sum() < n and not one["q"][~sky].any()
    a = abi.RadianceArgs()
    a.rays, a.sum, a.samples_per_ray = rays.data_ptr(), rays.data_ptr(), 1  # (n = 0: nothing is read or written)
    assert lib().rt_radiance_rays(ds.handle, C.byref(a), _stream()) == 0
    c = abi.CameraRaysArgs()
    c.pixels, c.width, c.height = index.data_ptr(), 37, 21
    assert lib().rt_camera_rays(C.byref(c), _stream()) == 0
    # pixel indices at and beyond the frame's end, among valid ones
    pick = torch.tensor([0, 776, 777, 5, 0x7fffffff, -1, 776], dtype=torch.int32, device="cuda")
    p_rays, p_index = camera(name, "philox", 0, pixels=pick)
    assert np.array_equal(p_index.cpu().numpy(), pick.cpu().numpy())
    r, full = p_rays.cpu().numpy(), rays.cpu().numpy()
    for k, p in enumerate((0, 776, None, 5, None, None, 776)):
        if p is None:
            assert r[k].tolist() == [[0.0, 0.0, 0.0, 1.0], [0.0, 0.0, 0.0, 0.0]]
        else:
            assert r[k].tobytes() == full[p].tobytes()
    occ = ds.occluded(p_rays)
    torch.cuda.synchronize()
    assert not occ.cpu().numpy()[[2, 4, 5]].any()


def test_python_wrappers_equal_the_direct_calls():
    name = "c2_37x21"
    ds = device_scene(name)
    inp = frame_inputs(name)
    w, h = FRAMES[name][2]
    rays, index = camera(name, "philox", 2)
    w_rays, w_index = camera_rays(inp, w, h, jitter="philox", sample=2, seed=SEED)
    torch.cuda.synchronize()
    assert w_rays.cpu().numpy().tobytes() == rays.cpu().numpy().tobytes() and torch.equal(w_index, index)
    assert w_index.dtype == torch.int32 and tuple(w_rays.shape) == (w * h, 2, 4)
    c_rays, _ = camera(name, (0.5, 0.5))
    assert camera_rays(inp, w, h)[0].cpu().numpy().tobytes() == c_rays.cpu().numpy().tobytes()
    pick = [5, 700, 5, 123]
    s_rays, s_index = camera_rays(inp, w, h, pixels=pick, jitter="philox", sample=2, seed=SEED)
    assert s_index.cpu().tolist() == pick and s_rays.cpu().numpy().tobytes() == rays.cpu().numpy()[pick].tobytes()
    t = abi.Tiling(8, 2, 1, len(band_rows_of(h, 8, 2, 1)))
    assert torch.equal(camera_rays(inp, w, h, tiling=t)[1], camera(name, (0.5, 0.5), tiling=t)[1])
    bg = (tuple(inp.background_start), tuple(inp.background_end))
    direct = radiance(ds, name, rays, w * h, ids=index, base=2, samples=2, count_tests=None)
    mean = ds.radiance(rays, samples=2, depth=FRAMES[name][3], sample_base=2, stream_ids=index, seed=SEED, background=bg)
    total = ds.radiance(rays, samples=2, depth=FRAMES[name][3], sample_base=2, stream_ids=index, seed=SEED, background=bg,
                        mean=False)
    torch.cuda.synchronize()
    assert mean.cpu().numpy().tobytes() == direct["mean"].tobytes() and total.cpu().numpy().tobytes() == direct["sum"].tobytes()
    plain = ds.radiance(rays.cpu().numpy(), samples=2, depth=FRAMES[name][3], sample_base=2, seed=SEED, background=bg)
    assert torch.equal(plain, mean)  # (numpy rays are uploaded; without ids ray i draws from stream i)
    ltr = ds.radiance(rays, depth=FRAMES[name][3], stream_ids=index, seed=SEED, background=bg, left_to_right=True)
    assert not torch.equal(ltr, ds.radiance(rays, depth=FRAMES[name][3], stream_ids=index, seed=SEED, background=bg))
    assert tuple(ds.radiance(rays[:0]).shape) == (0, 4)
    assert tuple(camera_rays(inp, w, h, pixels=[])[0].shape) == (0, 2, 4)
    with pytest.raises(ValueError):
        ds.radiance(rays.reshape(-1, 4))
    with pytest.raises(ValueError):
        ds.radiance(rays, stream_ids=index[:5])
    with pytest.raises(ValueError):
        camera_rays(inp, w, h, jitter="sobol")
