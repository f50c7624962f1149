"""rt_query_rays on the GPU, and rt_gbuffer / rt_trace_rays on a scene with 32-bit BVH references.

Scenes: the built-in RTIOW scene (16-bit references) and sphere_field(9000, 6) (32-bit: from its `hits` the test asserts
that a returned BVH index is >= 8192, so the references' upper bits are exercised).  Rays: the numpy centre rays of
40x24 and 37x21 frames under two 20-degree cameras (tests/test_query_host.py, query_case), uploaded as they are, so
kernel and reference trace the same rays; the far camera's frames are all sky on RTIOW and 46 % sky on the sphere
field.  Records are compared with the numpy reference on decidable rays (test_gpu_gbuffer.py's rule and its bounds for
t, the normal and the albedo); for (u, v) the bound is 4 · d with d the frame's float32-against-float64 spread of the
reference itself (uv_spread; 2.9e-5 .. 1.1e-3 on these frames, largest where rays graze the 1000-unit ground sphere
near its pole)."""
from __future__ import annotations

import ctypes as C

import numpy as np
import pytest
import torch

from cudaraytracer_amd import abi, scenes
from cudaraytracer_amd._lib import lib
from cudaraytracer_amd.renderer import DeviceScene, Renderer

from test_denoise_host import UNDECIDABLE_CAP, gbuffer_reference
from test_query_host import QUERY_SIZES, query_cameras, query_case, query_scene, uv_spread

pytestmark = pytest.mark.gpu

OUTPUTS = {"normal_depth": (4, torch.float32), "albedo": (4, torch.float32), "prim_id": (1, torch.int32),
           "uv": (2, torch.float32), "material": (1, torch.int32), "hits": (2, torch.int32)}
GUARD = 4    # guard elements before and after every output (whole 16-byte units for every element type)
FILL = 0x5a  # byte the outputs and their guards are filled with
FRAMES = [(camera, size) for camera in ("near", "far") for size in QUERY_SIZES]

_device_scenes = {}


def device_scene(name: str) -> DeviceScene:
    if name not in _device_scenes:
        _device_scenes[name] = DeviceScene(query_scene(name))
    return _device_scenes[name]


def prim_source(name: str) -> np.ndarray:
    """Per primitive in BVH order the hittable's index in the description (rt_build_host_tables)."""
    desc = query_scene(name).desc()
    info = abi.HostTablesInfo()
    assert lib().rt_build_host_tables(C.byref(desc), None, None, None, None, C.byref(info)) == 0
    nodes = (C.c_float * (16 * max(1, info.num_nodes)))()
    prims = (C.c_float * (8 * max(1, info.num_prims)))()
    mats = (C.c_float * (12 * max(1, info.num_materials)))()
    src = (C.c_int32 * max(1, info.num_prims))()
    assert lib().rt_build_host_tables(C.byref(desc), nodes, prims, mats, src, C.byref(info)) == 0
    return np.array(src[: info.num_prims], dtype=np.int32)


def query(ds: DeviceScene, rays: torch.Tensor, n: int, outputs=tuple(OUTPUTS), rays_per_lane: int = 0) -> dict:
    """One direct rt_query_rays call on the first n rays: {name: numpy array of n elements}, after checking that the
    GUARD elements before and after every output kept their fill."""
    bufs, a = {}, abi.QueryArgs()
    a.rays = rays.data_ptr()
    for name in outputs:
        width, dtype = OUTPUTS[name]
        bufs[name] = torch.full(((n + 2 * GUARD) * width * 4,), FILL, dtype=torch.uint8, device="cuda")
        setattr(a, name, bufs[name].data_ptr() + GUARD * width * 4)
    a.n, a.rays_per_lane = n, rays_per_lane
    rc = lib().rt_query_rays(ds.handle, C.byref(a), C.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0, (rc, lib().rt_last_error())
    torch.cuda.synchronize()
    out = {}
    for name in outputs:
        width, dtype = OUTPUTS[name]
        raw = bufs[name].cpu().numpy().reshape(n + 2 * GUARD, width * 4)
        assert np.all(raw[:GUARD] == FILL) and np.all(raw[n + GUARD:] == FILL), name
        body = raw[GUARD:n + GUARD]
        out[name] = body.copy().view(np.float32 if dtype == torch.float32 else np.int32).reshape((n, width) if width > 1 else (n,))
    return out


def same_bits(a: dict, b: dict, n: int | None = None) -> None:
    for name in a:
        assert a[name][:n].tobytes() == b[name][:n].tobytes(), name


def trace_rays(ds: DeviceScene, rays: torch.Tensor, n: int) -> np.ndarray:
    hits = torch.full((n, 2), -7, dtype=torch.int32, device="cuda")
    assert lib().rt_trace_rays(ds.handle, C.c_void_p(rays.data_ptr()), n, C.c_void_p(hits.data_ptr()), None, 0,
                               C.c_void_p(torch.cuda.current_stream().cuda_stream)) == 0, lib().rt_last_error()
    torch.cuda.synchronize()
    return hits.cpu().numpy()


def check_records(ref: dict, got: dict, traced: np.ndarray, src: np.ndarray, label: str, records: bool = True) -> None:
    """Checks 1-3 of one rt_query_rays launch `got` (all six outputs) on the rays of `ref`: `hits` is `traced`,
    rt_trace_rays' output for the same rays, bit for bit; the other outputs are consistent with `hits` (t bits,
    src[index] with src = the scene's prim_source, the misses' fill); and the records match the numpy reference `ref` on
    decidable rays.  records=False: of the reference only prim_id is compared."""
    hits = got["hits"]
    # 1. rt_trace_rays
    assert hits.tobytes() == traced.tobytes()
    # 2. consistency
    hit = hits[:, 0] >= 0
    assert hits[:, 0].max(initial=-1) < len(src)
    assert got["normal_depth"][hit, 3].tobytes() == hits[hit, 1].view(np.float32).tobytes()
    assert np.array_equal(got["prim_id"][hit], src[hits[hit, 0]])
    assert np.all(got["albedo"][hit, 3] == 1.0)
    assert np.all(hits[~hit, 0] == -1)
    nm = int((~hit).sum())
    assert np.array_equal(got["normal_depth"][~hit], np.broadcast_to(np.float32([0, 0, 0, -1]), (nm, 4)))
    assert not got["albedo"][~hit].any() and not got["uv"][~hit].any()
    assert np.all(got["prim_id"][~hit] == -1) and np.all(got["material"][~hit] == -1)
    # 3. the reference
    dec = ref["decidable"]
    share = 1.0 - float(dec.mean())
    assert share <= UNDECIDABLE_CAP, share
    wrong = dec & (got["prim_id"] != ref["prim_id"])
    assert not wrong.any(), (int(wrong.sum()), np.nonzero(wrong)[0][:5], got["prim_id"][wrong][:5], ref["prim_id"][wrong][:5])
    if not records:
        print(f"{label}: undecidable {share:.4f}, hits {hit.mean():.3f}, max index {hits[:, 0].max(initial=-1)}")
        return
    sel = dec & (ref["prim_id"] >= 0)
    d = uv_spread(ref)
    e_t = e_n = e_a = e_uv = 0.0
    if sel.any():
        t, t_ref = got["normal_depth"][sel, 3], ref["normal_depth"][sel, 3]
        e_t = float(np.max(np.abs(t - t_ref) / t_ref))
        e_n = float(np.max(np.abs(got["normal_depth"][sel, :3] - ref["normal_depth"][sel, :3])))
        e_a = float(np.max(np.abs(got["albedo"][sel] - ref["albedo"][sel])))
        e_uv = float(np.max(np.abs(got["uv"][sel] - ref["uv"][sel])))
    print(f"{label}: undecidable {share:.4f}, hits {hit.mean():.3f}, max index {hits[:, 0].max(initial=-1)}, "
          f"t rel {e_t:.2e}, normal {e_n:.2e}, albedo {e_a:.2e}, uv {e_uv:.2e} (d {d:.2e})")
    assert e_t <= 1e-4 and e_n <= 1e-4 and e_a <= 1e-4, (e_t, e_n, e_a)
    assert e_uv <= 4.0 * d, (e_uv, d)
    assert np.array_equal(got["material"][dec], ref["material"][dec])


@pytest.mark.parametrize("scene", ["rtiow", "wide"])
@pytest.mark.parametrize("camera,size", FRAMES)
def test_records(scene, camera, size):
    """Checks 1-3 (check_records): `hits` is rt_trace_rays' output bit for bit; the other outputs are consistent with
    `hits` (t bits, prim_source[index], the misses' fill); and the records match the numpy reference on decidable rays."""
    ref = query_case(scene, camera, size)
    ds = device_scene(scene)
    n = ref["rays"].shape[0]
    rays = torch.from_numpy(ref["rays"].copy()).cuda()
    got = query(ds, rays, n)
    check_records(ref, got, trace_rays(ds, rays, n), prim_source(scene), f"{scene} {camera} {size[0]}x{size[1]}")
    if scene == "wide" and camera == "far":  # (the upper reference bits are exercised: about 300 of these rays)
        assert got["hits"][:, 0].max() >= 8192, got["hits"][:, 0].max()


def gbuffer_planes(ds: DeviceScene, inputs, width: int, height: int, **tiling) -> tuple:
    r = Renderer(width, height, **tiling)
    nd, alb, prim = r.gbuffer(ds, inputs)
    torch.cuda.synchronize()
    return nd.cpu().numpy(), alb.cpu().numpy(), prim.cpu().numpy(), r.rows


def test_gbuffer_on_a_wide_scene():
    """Check 4: rt_gbuffer on the scene with 32-bit references against gbuffer_reference, under test_gpu_gbuffer.py's
    rule; a band render's rows equal the whole frame's."""
    scene, inputs, (w, h) = query_scene("wide"), query_cameras()["far"], QUERY_SIZES[0]
    ds = device_scene("wide")
    ref = gbuffer_reference(scene, inputs, w, h)
    nd, alb, prim, _ = whole = gbuffer_planes(ds, inputs, w, h)
    dec = ref["decidable"]
    share = 1.0 - float(dec.mean())
    assert share <= UNDECIDABLE_CAP, share
    wrong = dec & (prim != ref["prim_id"])
    assert not wrong.any(), (int(wrong.sum()), np.argwhere(wrong)[:5])
    hit, miss = dec & (ref["prim_id"] >= 0), dec & (ref["prim_id"] < 0)
    assert hit.any() and miss.any()
    t, t_ref = nd[..., 3][hit], ref["normal_depth"][..., 3][hit]
    e_t = float(np.max(np.abs(t - t_ref) / t_ref))
    e_n = float(np.max(np.abs(nd[..., :3][hit] - ref["normal_depth"][..., :3][hit])))
    e_a = float(np.max(np.abs(alb[dec] - ref["albedo"][dec])))
    print(f"wide far {w}x{h}: undecidable {share:.4f}, t rel {e_t:.2e}, normal {e_n:.2e}, albedo {e_a:.2e}")
    assert e_t <= 1e-4 and e_n <= 1e-4 and e_a <= 1e-4, (e_t, e_n, e_a)
    assert np.all(alb[..., 3] == 1.0)
    assert np.array_equal(nd[miss], np.broadcast_to(np.float32([0, 0, 0, -1]), nd[miss].shape))
    assert np.all(prim[miss] == -1)
    seen = []
    for rank in (0, 1):
        part = gbuffer_planes(ds, inputs, w, h, band_rows=8, num_ranks=2, rank=rank)
        rows = part[3]
        seen += rows
        for a, b in zip(part[:3], whole[:3]):
            assert a.tobytes() == b[rows].tobytes()
    assert sorted(seen) == list(range(h))


@pytest.mark.parametrize("scene,camera", [("rtiow", "near"), ("wide", "far")])
def test_ray_counts_and_refill(scene, camera):
    """Check 5: n = 1, 63, 65, 200, 960 with 1 and 4 rays per lane (at n = 200 with 4, one wave refills and its range
    ends mid-wave): the same bits for both settings — the whole batch's first n records — and untouched guards."""
    ref = query_case(scene, camera, QUERY_SIZES[0])
    ds = device_scene(scene)
    rays = torch.from_numpy(ref["rays"].copy()).cuda()
    assert rays.shape[0] == 960
    whole = query(ds, rays, 960)
    for n in (1, 63, 65, 200, 960):
        one = query(ds, rays, n, rays_per_lane=1)
        four = query(ds, rays, n, rays_per_lane=4)
        same_bits(one, four)
        same_bits(one, whole, n)
    same_bits(query(ds, rays, 960, rays_per_lane=16), whole)


def test_optional_outputs_determinism_and_aliasing():
    """Check 6: each output alone gives the bits it has among all six; two calls give the same bits; a call whose
    outputs alias is rejected and writes nothing."""
    ref = query_case("wide", "far", QUERY_SIZES[1])
    ds = device_scene("wide")
    n = ref["rays"].shape[0]
    rays = torch.from_numpy(ref["rays"].copy()).cuda()
    full = query(ds, rays, n)
    same_bits(query(ds, rays, n), full)
    for name in OUTPUTS:
        alone = query(ds, rays, n, outputs=(name,))
        assert alone[name].tobytes() == full[name].tobytes(), name
    buf = torch.full((n * 16 + 64,), FILL, dtype=torch.uint8, device="cuda")
    before = rays.clone()
    a = abi.QueryArgs()
    a.rays, a.n = rays.data_ptr(), n
    a.normal_depth = buf.data_ptr()
    a.prim_id = buf.data_ptr() + n * 16 - 16  # inside normal_depth
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    assert lib().rt_query_rays(ds.handle, C.byref(a), stream) == -1
    assert b"rt_query_rays" in lib().rt_last_error() and b"overlap" in lib().rt_last_error()
    a.prim_id = None
    a.hits = rays.data_ptr() + 32  # inside the rays
    assert lib().rt_query_rays(ds.handle, C.byref(a), stream) == -1
    assert b"overlaps rays" in lib().rt_last_error()
    torch.cuda.synchronize()
    assert bool((buf == FILL).all()) and torch.equal(rays, before)


def test_device_scene_query_equals_the_direct_call():
    """Check 7: DeviceScene.query, from a device tensor and from a numpy array, with all outputs and with a subset."""
    ref = query_case("wide", "far", QUERY_SIZES[1])
    ds = device_scene("wide")
    n = ref["rays"].shape[0]
    rays = torch.from_numpy(ref["rays"].copy()).cuda()
    full = query(ds, rays, n)
    for given in (rays, ref["rays"]):
        out = ds.query(given)
        torch.cuda.synchronize()
        assert set(out) == set(OUTPUTS)
        for name, (width, dtype) in OUTPUTS.items():
            assert out[name].dtype == dtype and tuple(out[name].shape) == ((n, width) if width > 1 else (n,))
            assert out[name].cpu().numpy().tobytes() == full[name].tobytes(), name
    out = ds.query(rays, outputs=("prim_id", "uv"), rays_per_lane=4)
    torch.cuda.synchronize()
    assert set(out) == {"prim_id", "uv"}
    assert out["uv"].cpu().numpy().tobytes() == full["uv"].tobytes()
    assert out["prim_id"].cpu().numpy().tobytes() == full["prim_id"].tobytes()
    assert ds.query(rays[:0])["hits"].shape == (0, 2)
    with pytest.raises(ValueError):
        ds.query(rays, outputs=("depth",))
    with pytest.raises(ValueError):
        ds.query(rays.reshape(-1, 4))


def test_empty_scene_gives_all_misses():
    """A description with every hittable switched off: every ray misses."""
    s = scenes.builtin(scenes.SCENE_THREE_SPHERES)
    for h in s.hittables:
        h.is_active = 0
    ds = DeviceScene(s)
    rays = torch.from_numpy(query_case("rtiow", "near", QUERY_SIZES[1])["rays"].copy()).cuda()
    got = query(ds, rays, 100)
    assert np.all(got["hits"][:, 0] == -1) and np.all(got["prim_id"] == -1) and np.all(got["material"] == -1)
    assert np.array_equal(got["normal_depth"], np.broadcast_to(np.float32([0, 0, 0, -1]), (100, 4)))
    assert not got["albedo"].any() and not got["uv"].any()


def test_viewer_passes_on_a_wide_scene():
    """Check 8: render -> gbuffer -> temporal(moments=True) -> denoise_variance on the scene with 32-bit references,
    two frames, returns RT_OK (the wrappers raise otherwise) and finite planes."""
    w, h = 64, 40
    inputs = scenes.CONFIGS["c2"].inputs()
    ds = device_scene("wide")
    r = Renderer(w, h)
    r.render_init()
    for _ in range(2):
        r.render(ds, 1, 4, inputs, radiance=True)
        nd, alb, prim = r.gbuffer(ds, inputs, keep_previous=True)
        r.temporal(moments=True)
        img = r.denoise_variance()
    torch.cuda.synchronize()
    assert img.shape == (h, w)
    assert int(prim.max()) >= 1 and int(prim.min()) >= -1
    for plane in (nd, alb, r.history, r.moments, r.denoised_variance):
        assert bool(torch.isfinite(plane).all())
    assert float(r.history[..., 3].min()) >= 1.0
