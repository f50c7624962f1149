"""rt_radiance_rays with RT_RADIANCE_DIRECT_LIGHT on the GPU.

Direct C calls, the outputs inside 0x5a-filled buffers with 16 guard elements on either side (tests/test_gpu_radiance.py's
helpers).  What is checked: where there is nothing to sample the flag changes no bit; the direct term itself against a
numpy float32 restatement built from the oracle's hit test and Philox words; its expectation against a float64
quadrature (and against the flagless estimator, which must meet the same bound); the whole estimator against the
flagless one on the Cornell box; that it lowers the error there; and the schedule and composition rules of the call.

Tolerances.  Test 2: one 2^-12 unit — the restatement's y, v and shadow ray are the kernel's bit for bit (separately
rounded operations in the header's order), the weight's products are not promised in one order, and a relative 2^-20
of a value below 2 is under a tenth of a unit, so only a rounding boundary can move the quantised value, by one.
Tests 3 and 4: five standard errors of the 32 call means, plus 2^-13 in test 3 for the quantisation's half unit."""
from __future__ import annotations

import ctypes as C
import functools

import numpy as np
import pytest
import torch

from cudaraytracer_amd import abi, scenes
from cudaraytracer_amd._lib import lib
from cudaraytracer_amd.renderer import DeviceScene, camera_rays
from oracle import py_oracle as po

from test_denoise_host import FLT_MAX
from test_direct_light_host import (DIRECT, FLOOR_POINT, LAMP_CENTER, LAMP_SIZE, lamp_quadrature, lights_of, make_scene, material,
                                    rect, sphere)
from test_gpu_radiance import GUARD, _body, _guarded, _stream, camera, device_scene
from test_query_host import query_cameras, query_scene
from test_radiance_host import FRAMES, SEED, frame_inputs, frame_scene

pytestmark = pytest.mark.gpu

F = np.float32
BLACK = ((0.0, 0.0, 0.0), (0.0, 0.0, 0.0))
ALBEDO = (0.5, 0.25, 0.125)


def trace(ds: DeviceScene, rays: torch.Tensor, depth: int, flags: int = 0, n: int | None = None, ids: torch.Tensor | None = None,
          base: int = 0, samples: int = 1, rays_per_lane: int = 0, count_tests: int = 0, stream_base: int = 0, frame: int = 0,
          background=BLACK) -> dict:
    """One direct rt_radiance_rays call: {"sum", "mean": (n, 4) float32, "q": sum.rgb in 2^-12 units, "counters"}, after
    checking the guards."""
    n = rays.shape[0] if n is None else n
    a = abi.RadianceArgs()
    a.rays = rays.data_ptr()
    bufs = {o: _guarded(n, 16) for o in ("sum", "mean")}
    for o, b in bufs.items():
        setattr(a, o, b.data_ptr() + GUARD * 16)
    if ids is not None:
        a.stream_ids = ids.data_ptr()
    a.n, a.rays_per_lane, a.samples_per_ray, a.sample_base, a.max_depth = n, rays_per_lane, samples, base, depth
    a.flags, a.stream_base, a.rng_seed, a.rng_frame = flags, stream_base, SEED, frame
    a.background_start[:] = list(background[0])
    a.background_end[:] = list(background[1])
    counters = torch.zeros(abi.COUNTERS_WORDS, dtype=torch.int64, device="cuda")
    a.counters, a.count_tests = counters.data_ptr(), count_tests
    rc = lib().rt_radiance_rays(ds.handle, C.byref(a), _stream())
    assert rc == 0, (rc, lib().rt_last_error())
    torch.cuda.synchronize()
    out = {o: _body(bufs[o], n, 16, o).view(F).reshape(n, 4) for o in bufs}
    assert np.all(out["sum"][:, 3] == F(samples)) and np.all(out["mean"][:, 3] == F(1.0))
    units = out["sum"][:, :3].astype(np.float64) * 4096.0
    assert np.all(units == np.round(units))
    out["q"] = units.astype(np.uint64)
    out["counters"] = counters.cpu().numpy()
    return out


def same_bits(a: dict, b: dict) -> None:
    assert a["sum"].tobytes() == b["sum"].tobytes() and a["mean"].tobytes() == b["mean"].tobytes()


def frame_background(name: str) -> tuple:
    inp = frame_inputs(name)
    return (tuple(inp.background_start), tuple(inp.background_end))


def down_rays(points) -> np.ndarray:
    """Rays straight down from y = 0.5 onto floor points (x, z)."""
    pts = np.asarray(points, dtype=F)
    rays = np.zeros((len(pts), 2, 4), dtype=F)
    rays[:, 0, 0], rays[:, 0, 1], rays[:, 0, 2] = pts[:, 0], F(0.5), pts[:, 1]
    rays[:, 1, 1] = F(-1.0)
    return rays


# ---------------------------------------------------------------------------------------------------------------------
# 1. Nothing to sample: the same bits
# ---------------------------------------------------------------------------------------------------------------------
def _metal_c3() -> scenes.Scene:
    s = scenes.Scene.from_bytes(frame_scene("c3").hittables_bytes(), frame_scene("c3").materials_bytes())
    swapped = 0
    for m in s.materials:
        if m.type == abi.RT_LAMBERTIAN:
            m.type, m.fuzz = abi.RT_METAL, 0.3
            swapped += 1
    assert swapped >= 3 and lights_of(s) == (1, [2])
    return s


@pytest.mark.parametrize("case", ["c2_37x21", "c5", "c3_metal", "c3_depth1"])
def test_nothing_to_sample_changes_no_bit(case):
    """No sampled light (c2, c5: the kernel is the flagless one), lights but no diffuse vertex (c3 in metal), and lights
    but no vertex that may connect (c3 at max_depth 1): sum, mean and counters equal the flagless call's."""
    name = {"c3_metal": "c3", "c3_depth1": "c3"}.get(case, case)
    ds = DeviceScene(_metal_c3()) if case == "c3_metal" else device_scene(name)
    depth = 1 if case == "c3_depth1" else FRAMES[name][3]
    if name != "c3":
        assert lights_of(frame_scene(name))[0] == 0
    orders = (0, abi.RT_FLAG_RIUS_LEFT_TO_RIGHT) if case in ("c2_37x21", "c3_metal") else (0,)
    rays, index = camera(name, "philox", 0)
    results = []
    for order in orders:
        for count in (0, 1):
            plain = trace(ds, rays, depth, order, ids=index, samples=2, count_tests=count, background=frame_background(name))
            flagged = trace(ds, rays, depth, order | DIRECT, ids=index, samples=2, count_tests=count,
                            background=frame_background(name))
            same_bits(flagged, plain)
            assert int(plain["counters"][0]) > 0 and int(plain["counters"][3]) == 2 * rays.shape[0]
            if case in ("c2_37x21", "c5") or count == 0:  # (the same kernel, or the words every build writes)
                assert np.array_equal(flagged["counters"], plain["counters"])
            assert np.array_equal(flagged["counters"][[0, 3]], plain["counters"][[0, 3]])
        results.append(plain["sum"].tobytes())
        assert plain["q"].any()
    assert len(set(results)) == len(orders)  # (the fill order matters on these frames)
    if case == "c3_metal":
        ds.close()


# ---------------------------------------------------------------------------------------------------------------------
# 2. The direct term, deterministically
# ---------------------------------------------------------------------------------------------------------------------
def floor_scene(with_extras: bool = True) -> scenes.Scene:
    mats = [material(abi.RT_LAMBERTIAN, ALBEDO), material(abi.RT_DIFFUSELIGHT, (1.0, 1.0, 1.0), 4),
            material(abi.RT_DIFFUSELIGHT, (1.0, 0.5, 0.25), 6), material(abi.RT_LAMBERTIAN, (0.7, 0.7, 0.7))]
    hs = [rect(abi.RT_XZRECT, (0.0, 0.0, 0.0), 10.0, 10.0, 0), rect(abi.RT_XZRECT, LAMP_CENTER, LAMP_SIZE[0], LAMP_SIZE[1], 1)]
    if with_extras:
        hs += [rect(abi.RT_XZRECT, (-1.0, 1.5, 0.5), 0.3, 0.3, 2), sphere((0.45, 0.75, 0.15), 0.12, 3)]
    return make_scene(hs, mats)


GRID = [(x, z) for z in np.linspace(0.3, 1.5, 7) for x in np.linspace(-1.6, 1.6, 9)]  # 9 x 7 floor points, none under a lamp
TERM_SAMPLES = 8


def _f3(v) -> np.ndarray:
    return np.array([v[0], v[1], v[2]], dtype=F)


@functools.lru_cache(maxsize=None)
def direct_term_reference() -> dict:
    """The restatement: for every ray of GRID and sample 0..7, a * D in 2^-12 units and what kind of connection it was."""
    scene = floor_scene()
    L = po.lib()
    lights = lights_of(scene)[1]
    assert lights == [1, 2]
    nl = len(lights)
    rays = down_rays(GRID)
    ids = (1000 + 7 * np.arange(len(GRID))).astype(np.uint32)
    fp = C.POINTER(C.c_float)
    want = np.zeros((TERM_SAMPLES, len(GRID), 3), dtype=np.uint64)
    kind = np.zeros((TERM_SAMPLES, len(GRID)), dtype=np.int32)  # 1 free, 2 occluded, 3 c <= 0 or c' <= 0
    lamp = np.zeros((TERM_SAMPLES, len(GRID)), dtype=np.int32)
    rec = po.Hit()
    for i in range(len(GRID)):
        o, d = np.ascontiguousarray(rays[i, 0, :3]), np.ascontiguousarray(rays[i, 1, :3])
        assert L.orc_hittable_hit(C.byref(scene.hittables[0]), o.ctypes.data_as(fp), d.ctypes.data_as(fp), F(0.001), F(FLT_MAX),
                                  C.byref(rec))
        for k in (2, 3):  # (the camera ray meets the floor first)
            other = po.Hit()
            assert not L.orc_hittable_hit(C.byref(scene.hittables[k]), o.ctypes.data_as(fp), d.ctypes.data_as(fp), F(0.001),
                                          F(rec.t), C.byref(other))
        P, nrm = _f3(rec.p), _f3(rec.normal)
        assert nrm.tolist() == [0.0, 1.0, 0.0] and P[1] == 0
        for s in range(TERM_SAMPLES):
            block = (s << 16) + 65535
            xi = [F(L.orc_philox_uniform_at(SEED, int(ids[i]), 0, 4 * block + w)) for w in range(3)]
            l = min(int(np.uint32(xi[0] * F(nl))), nl - 1)
            h = scene.hittables[lights[l]]
            m = scene.materials[h.material]
            y = _f3(h.center)
            y[0] = y[0] + (xi[1] - F(0.5)) * F(h.width)   # XZ: width along x, height along z
            y[2] = y[2] + (xi[2] - F(0.5)) * F(h.height)
            v = y - P
            d2 = F(F(v[0] * v[0] + v[1] * v[1]) + v[2] * v[2])
            dist = np.sqrt(d2, dtype=F)
            c = F(F(nrm[0] * v[0] + nrm[1] * v[1]) + nrm[2] * v[2]) / dist
            cp = np.abs(v[1]) / dist
            lamp[s, i] = l
            if not (c > 0 and cp > 0):
                kind[s, i] = 3
                continue
            blocked = False
            vv = np.ascontiguousarray(v)
            for hh in scene.hittables:
                blocked |= bool(L.orc_hittable_hit(C.byref(hh), P.ctypes.data_as(fp), vv.ctypes.data_as(fp), F(1e-4), F(0.9999),
                                                   C.byref(po.Hit())))
            if blocked:
                kind[s, i] = 2
                continue
            kind[s, i] = 1
            g = F(2.0) * (c * c * c) * cp * F(F(h.width) * F(h.height)) * F(nl) / F(F(3.141592654) * d2)
            le = F(m.light_intensity) * _f3(m.albedo.color)
            term = _f3(ALBEDO) * (F(g) * le)
            want[s, i] = (term.astype(F) * F(4096.0) + F(0.5)).astype(np.uint64)
    out = {"rays": rays, "ids": ids, "want": want, "kind": kind, "lamp": lamp}
    for a in out.values():
        a.setflags(write=False)
    return out


def test_direct_term_equals_its_restatement():
    ref = direct_term_reference()
    kind, lamp, want = ref["kind"], ref["lamp"], ref["want"]
    # the restatement covers the cases: free and occluded connections, both lamps (each free somewhere), and — the floor
    # faces both lamps — no connection with c <= 0
    assert (kind == 1).sum() > 100 and (kind == 2).sum() >= 3 and (kind == 3).sum() == 0
    assert set(lamp[kind == 1].tolist()) == {0, 1} and set(lamp[kind == 2].tolist()) == {0}
    assert want[kind == 1].any(axis=1).mean() > 0.9 and not want[kind == 2].any()  # (a far, grazing connection rounds to 0)
    ds = DeviceScene(floor_scene())
    rays, ids = torch.from_numpy(ref["rays"].copy()).cuda(), torch.from_numpy(ref["ids"].view(np.int32).copy()).cuda()
    worst, shadow_rays = 0, 0
    for s in range(TERM_SAMPLES):
        got = trace(ds, rays, 2, DIRECT, ids=ids, base=s)
        plain = trace(ds, rays, 2, 0, ids=ids, base=s)
        diff = np.abs(got["q"].astype(np.int64) - want[s].astype(np.int64))
        worst = max(worst, int(diff.max()))
        print(f"sample {s}: largest difference {int(diff.max())} unit(s), free {(kind[s] == 1).sum()}, occluded {(kind[s] == 2).sum()}")
        assert diff.max() <= 1, (s, np.argwhere(diff > 1)[:4])
        assert not got["q"][kind[s] == 2].any()
        # one shadow ray per connection that could count, blocked or not, beside the path's two rays
        assert int(plain["counters"][0]) == 2 * len(GRID) and int(plain["counters"][3]) == len(GRID)
        assert int(got["counters"][0]) - int(plain["counters"][0]) == int((kind[s] != 3).sum())
        assert int(got["counters"][3]) == len(GRID)
        shadow_rays += int((kind[s] != 3).sum())
    assert shadow_rays == TERM_SAMPLES * len(GRID)
    ds.close()


# ---------------------------------------------------------------------------------------------------------------------
# 3. Against quadrature
# ---------------------------------------------------------------------------------------------------------------------
CALLS, CALL_SAMPLES = 32, 512


def call_means(ds, rays, depth, flags, ids=None, background=BLACK) -> np.ndarray:
    """(CALLS, n, 3) float64: the mean of CALL_SAMPLES samples per ray for rng_frame 0 .. CALLS - 1."""
    out = []
    for frame in range(CALLS):
        r = trace(ds, rays, depth, flags, ids=ids, samples=CALL_SAMPLES, frame=frame, rays_per_lane=1, background=background)
        out.append(r["q"].astype(np.float64) / 4096.0 / CALL_SAMPLES)
    return np.array(out)


def test_expectation_equals_the_quadrature():
    points = [(FLOOR_POINT[0], FLOOR_POINT[2]), (1.2, 0.5), (-0.5, -0.8)]
    ds = DeviceScene(floor_scene(with_extras=False))
    rays = torch.from_numpy(down_rays(points)).cuda()
    want = np.array([[a * 4.0 * lamp_quadrature((x, 0.0, z)) for a in ALBEDO] for x, z in points])
    for flags in (DIRECT, 0):  # (the flagless call is the brute-force estimator: the bound is not vacuous)
        means = call_means(ds, rays, 2, flags)
        mean, se = means.mean(axis=0), means.std(axis=0, ddof=1) / np.sqrt(CALLS)
        print(f"flags {flags}: mean {mean.tolist()} se {se.tolist()} quadrature {want.tolist()}")
        assert np.all(se > 0)
        assert np.all(np.abs(mean - want) <= 5 * se + 2.0 ** -13), (flags, mean, want, se)
    ds.close()


# ---------------------------------------------------------------------------------------------------------------------
# 4. Unbiased on C3
# ---------------------------------------------------------------------------------------------------------------------
def test_unbiased_on_the_cornell_box():
    w, h = 24, 16
    inp = scenes.CONFIGS["c3"].inputs()
    rays, index = camera_rays(inp, w, h)  # centre jitter
    ds = device_scene("c3")
    bg = frame_background("c3")

    def blocks(flags):
        m = call_means(ds, rays, 6, flags, ids=index, background=bg).sum(axis=2)            # (CALLS, n): r + g + b
        m = m.reshape(CALLS, h // 4, 4, w // 4, 4).mean(axis=(2, 4)).reshape(CALLS, -1)   # (CALLS, 24 blocks)
        return m.mean(axis=0), m.std(axis=0, ddof=1) / np.sqrt(CALLS)

    mean_f, se_f = blocks(DIRECT)
    mean_p, se_p = blocks(0)
    print("plain SE / mean per block:", np.round(se_p / mean_p, 4).tolist())
    print("flagged SE / mean per block:", np.round(se_f / mean_f, 4).tolist())
    assert np.all(se_p <= 0.05 * mean_p)  # the test has power in every block
    assert np.all(np.abs(mean_f - mean_p) <= 5 * np.sqrt(se_f ** 2 + se_p ** 2)), (mean_f, mean_p)


# ---------------------------------------------------------------------------------------------------------------------
# 5. Lower error
# ---------------------------------------------------------------------------------------------------------------------
def cornell_mse(samples_list=(64,)) -> dict:
    """{samples: (MSE flagless, MSE flagged)} of c3 32 x 32 at depth 8 against the flagless mean of 16384 samples (another
    rng_frame than the estimates')."""
    ds = device_scene("c3")
    bg = frame_background("c3")
    rays, index = camera("c3", (0.5, 0.5))
    ref = trace(ds, rays, 8, 0, ids=index, samples=abi.PHILOX_MAX_SPP, frame=0, rays_per_lane=1, background=bg)
    assert ref["q"].max() < 0xffffffff  # (no saturated sum)
    ref = ref["q"].astype(np.float64) / 4096.0 / abi.PHILOX_MAX_SPP
    out = {}
    for k in samples_list:
        mse = []
        for flags in (0, DIRECT):
            est = trace(ds, rays, 8, flags, ids=index, samples=k, frame=7, rays_per_lane=1, background=bg)
            mse.append(float(((est["q"].astype(np.float64) / 4096.0 / k - ref) ** 2).mean()))
        out[k] = tuple(mse)
    return out


def test_lower_error_on_the_cornell_box():
    plain, flagged = cornell_mse()[64]
    print(f"c3 32x32 depth 8, 64 samples: MSE flagless {plain:.6g}, flagged {flagged:.6g}, ratio {flagged / plain:.4f}")
    assert flagged < plain


# ---------------------------------------------------------------------------------------------------------------------
# 6. Schedule and composition
# ---------------------------------------------------------------------------------------------------------------------
def test_schedule_and_composition():
    ds = device_scene("c3")
    bg = frame_background("c3")
    rays, index = camera("c3", "philox", 0)
    n = rays.shape[0]
    whole = trace(ds, rays, 8, DIRECT, ids=index, base=1, samples=3, background=bg)
    assert not np.array_equal(whole["q"], trace(ds, rays, 8, 0, ids=index, base=1, samples=3, background=bg)["q"])
    for rpl in (0, 1, 16):
        same_bits(trace(ds, rays, 8, DIRECT, ids=index, base=1, samples=3, rays_per_lane=rpl, background=bg), whole)
    counted = trace(ds, rays, 8, DIRECT, ids=index, base=1, samples=3, count_tests=1, background=bg)
    same_bits(counted, whole)
    assert int(counted["counters"][0]) == int(whole["counters"][0]) and int(counted["counters"][1]) > 0
    for key, values in ((abi.RT_TUNE_REGEN_THRESHOLD, (1, 64)), (abi.RT_TUNE_LEAF_BREAK, (0, 64))):
        for v in values:
            prev = lib().rt_set_tuning(key, v)
            try:
                same_bits(trace(ds, rays, 8, DIRECT, ids=index, base=1, samples=3, rays_per_lane=3, background=bg), whole)
            finally:
                lib().rt_set_tuning(key, prev)
    parts = [trace(ds, rays, 8, DIRECT, ids=index, base=1 + k, background=bg) for k in range(3)]
    assert np.array_equal(whole["q"], np.minimum(sum(p["q"] for p in parts), np.uint64(0xffffffff)))
    assert len({p["q"].tobytes() for p in parts}) == 3
    for word in (0, 3):
        assert int(whole["counters"][word]) == sum(int(p["counters"][word]) for p in parts)
    assert int(whole["counters"][3]) == 3 * n
    # ids against stream_base: a dense frame's pixel indices are base 0 + i; another base is another stream
    assert np.array_equal(index.cpu().numpy(), np.arange(n, dtype=np.int32))
    same_bits(trace(ds, rays, 8, DIRECT, base=1, samples=3, background=bg), whole)
    shifted = (index + 500).contiguous()
    by_ids = trace(ds, rays, 8, DIRECT, ids=shifted, base=1, samples=3, background=bg)
    same_bits(trace(ds, rays, 8, DIRECT, base=1, samples=3, stream_base=500, background=bg), by_ids)
    assert by_ids["sum"].tobytes() != whole["sum"].tobytes()
    # the Python wrapper is the direct call
    wrapped = ds.radiance(rays, samples=3, depth=8, sample_base=1, stream_ids=index, seed=SEED, background=bg, direct_light=True)
    torch.cuda.synchronize()
    assert wrapped.cpu().numpy().tobytes() == whole["mean"].tobytes()


def _wide_with_rect(lamp: bool) -> scenes.Scene:
    """The wide-reference scene with a fifth material and one rectangle of it above the camera's view: Lambertian, or
    (lamp) a light."""
    base = query_scene("wide")
    mats = list(base.materials) + [material(abi.RT_DIFFUSELIGHT, (1.0, 0.9, 0.8), 8) if lamp
                                   else material(abi.RT_LAMBERTIAN, (0.5, 0.5, 0.5))]
    hs = list(base.hittables) + [rect(abi.RT_XZRECT, (0.0, 3.0, 0.0), 2.0, 2.0, 4)]
    return make_scene(hs, mats)


def test_material_update_rebuilds_the_light_list():
    name = "wide_near"
    plain_scene, lamp_scene = _wide_with_rect(False), _wide_with_rect(True)
    rect_index = len(plain_scene.hittables) - 1
    assert lights_of(plain_scene) == (0, []) and lights_of(lamp_scene) == (1, [rect_index])
    rays, index = camera(name, "philox", 0)
    bg = frame_background(name)
    ds = DeviceScene(plain_scene)
    assert ds.info().num_primitives >= 8192  # (32-bit references: the WIDE builds)
    before = trace(ds, rays, 6, DIRECT, ids=index, samples=2, background=bg)
    same_bits(before, trace(ds, rays, 6, 0, ids=index, samples=2, background=bg))  # (no light yet)
    ds.update_materials(lamp_scene.materials)
    after = trace(ds, rays, 6, DIRECT, ids=index, samples=2, background=bg)
    assert after["sum"].tobytes() != before["sum"].tobytes()
    fresh = DeviceScene(lamp_scene)
    want = trace(fresh, rays, 6, DIRECT, ids=index, samples=2, background=bg)
    same_bits(after, want)
    assert np.array_equal(after["counters"], want["counters"])
    assert int(after["counters"][0]) > int(trace(fresh, rays, 6, 0, ids=index, samples=2, background=bg)["counters"][0])
    # ... and back: the rectangle stops being a light, the flagged call is the flagless one again
    ds.update_materials(plain_scene.materials)
    same_bits(trace(ds, rays, 6, DIRECT, ids=index, samples=2, background=bg), before)
    # an edited copy (rt_scene_edit) carries the list too
    ds.update_materials(lamp_scene.materials)
    edited = ds.edited(lamp_scene.hittables)
    same_bits(trace(edited, rays, 6, DIRECT, ids=index, samples=2, background=bg), want)
    for d in (edited, fresh, ds):
        d.close()
