"""rt_query_rays, rt_trace_rays and rt_occluded_rays on rays of the caller's own: the families of tests/ray_families.py.

Axis-aligned rays with +0 and -0 components (the +-1e20 clamp of the reciprocal direction is the whole answer for them:
the per-ray kernels have no reference replay), directions with one zero or one subnormal component, waves whose 64
lanes start inside the scene in unrelated directions, ambient-occlusion ranges, and directions scaled by 2^-24 .. 2^21
— on four scenes: 16-bit and 32-bit BVH references, rectangles only, and every primitive and texture type.  Compared
with the brute-force reference on decidable rays (tests/test_ray_families_host.py asserts the families' properties on
the CPU), with rt_trace_rays, and with themselves across zero signs, scales and schedules, bit for bit.  Every case is a
launch or a few of at most 960 rays."""
from __future__ import annotations

import numpy as np
import pytest
import torch

import ray_families as rf
from cudaraytracer_amd.renderer import DeviceScene
from test_denoise_host import FLT_MAX, UNDECIDABLE_CAP
from test_gpu_occlusion import consistent, occluded, with_range
from test_gpu_occlusion import same_bits as same_occlusion_bits
from test_gpu_query import check_records, device_scene, query, same_bits, trace_rays
from test_occlusion_host import hittable_hits

pytestmark = pytest.mark.gpu

F = np.float32
_device_scenes, _sources = {}, {}


def device(name: str) -> DeviceScene:
    if name in ("wide", "rtiow"):  # (the query tests' own, not a second copy)
        return device_scene(name)
    if name not in _device_scenes:
        _device_scenes[name] = DeviceScene(rf.scene(name))
    return _device_scenes[name]


def source(name: str) -> np.ndarray:
    if name not in _sources:
        _sources[name] = rf.prim_source(rf.scene(name))
    return _sources[name]


def upload(rays: np.ndarray) -> torch.Tensor:
    return torch.from_numpy(np.array(rays, dtype=F)).cuda()


# ---------------------------------------------------------------------------------------------------------------------
# a. Records
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scene", rf.SCENES)
@pytest.mark.parametrize("family", rf.QUERY_FAMILIES)
def test_records(scene, family):
    """test_gpu_query.py's checks 1-3 (check_records): `hits` is rt_trace_rays' output bit for bit, the outputs are
    consistent with it, and on decidable rays prim_id and material are the reference's, t, normal and albedo within 1e-4
    and (u, v) within 4 · uv_spread.  tiny: prim_id only (a subnormal component is below what the reciprocal resolves:
    the kernel treats it as the zero of its sign)."""
    ref = rf.family_case(scene, family)
    ds = device(scene)
    n = ref["rays"].shape[0]
    rays = upload(ref["rays"])
    got = query(ds, rays, n)
    check_records(ref, got, trace_rays(ds, rays, n), source(scene), f"{scene} {family}", records=family != "tiny")
    if scene == "wide" and family in ("axis", "interior"):  # (the upper reference bits are exercised)
        assert got["hits"][:, 0].max() >= 8192, got["hits"][:, 0].max()


@pytest.mark.parametrize("scene", rf.SCENES)
def test_zero_signs_do_not_matter(scene):
    """-0 on the even indices in place of the odd ones: the same bits in every output, closest hit and occlusion."""
    ds = device(scene)
    a, b = rf.axis(scene), rf.axis(scene, neg_zero="even")
    assert a.tobytes() != b.tobytes() and np.array_equal(a, b)
    n = a.shape[0]
    same_bits(query(ds, upload(a), n), query(ds, upload(b), n))
    same_occlusion_bits(occluded(ds, upload(rf.axis_occ(scene)), n), occluded(ds, upload(rf.axis_occ(scene, "even")), n))


# ---------------------------------------------------------------------------------------------------------------------
# b. Occlusion
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scene", rf.SCENES)
@pytest.mark.parametrize("family", rf.OCCLUSION_FAMILIES)
def test_occlusion(scene, family):
    """`occluded` is the reference's on decidable rays; every blocker is a hittable whose own test accepts the ray over
    its range (on every ray, decidable or not)."""
    case = rf.family_case(scene, family)
    ds, desc = device(scene), rf.scene(scene)
    rays = case["rays"]
    n = rays.shape[0]
    got = occluded(ds, upload(rays), n)
    consistent(got, desc)
    dec = case["decidable"]
    share = 1.0 - float(dec.mean())
    occ = got["occluded"] == 1
    wrong = dec & (occ != case["occluded"])
    print(f"{scene} {family}: undecidable {share:.4f}, occluded {occ.mean():.3f} (reference {case['occluded'].mean():.3f}), "
          f"differing undecidable rays {int((~dec & (occ != case['occluded'])).sum())}")
    assert share <= UNDECIDABLE_CAP, share
    assert not wrong.any(), (int(wrong.sum()), np.nonzero(wrong)[0][:8])
    for r in np.nonzero(got["blocker"] >= 0)[0]:
        h = desc.hittables[int(got["blocker"][r])]
        assert hittable_hits(h, rays[r, 0, :3], rays[r, 1, :3], rays[r, 0, 3], rays[r, 1, 3]), (r, int(got["blocker"][r]))


@pytest.mark.parametrize("scene", rf.SCENES)
@pytest.mark.parametrize("family", ["axis", "planar", "interior"])
def test_occlusion_against_the_closest_hit(scene, family):
    """Over (0.001, FLT_MAX) a ray is occluded exactly when rt_trace_rays finds a hit: on every ray, a failure is a bug."""
    ds = device(scene)
    rays = with_range(rf.family_case(scene, family)["rays"], 0.001, FLT_MAX)
    n = rays.shape[0]
    hit = trace_rays(ds, rays, n)[:, 0] >= 0
    got = occluded(ds, rays, n)
    consistent(got, rf.scene(scene))
    assert np.array_equal(got["occluded"] == 1, hit), np.nonzero((got["occluded"] == 1) != hit)[0][:8]


# ---------------------------------------------------------------------------------------------------------------------
# c. Scaling
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scene", ["wide", "mixed"])
@pytest.mark.parametrize("family", ["interior", "axis"])
def test_scaled_directions_closest_hit(scene, family):
    """d · 2^k gives the primitive the unscaled ray gives and t · 2^k the unscaled t, bit for bit: a power of two commutes
    with every operation of the primitive tests (tests/test_ray_families_host.py shows it of the reference), div_rn is
    IEEE division, and the slab test scales exactly inside the header's magnitude range.  k = -19 keeps dot(d, d)
    inside [2^-40, 2^40], where the sphere roots use div_rn / rcp_rn; -21 and -24 take the IEEE sequence.  k = +6: rays
    whose unscaled t exceeds 0.25, and the misses (the fixed tmin of 0.001 is 0.064 in the unscaled ray's units)."""
    ds = device(scene)
    base_rays = rf.family_case(scene, family)["rays"]
    n = base_rays.shape[0]
    base = query(ds, upload(base_rays), n, outputs=("hits",))["hits"]
    hit = base[:, 0] >= 0
    t0 = base[:, 1].copy().view(F)
    assert hit.mean() > 0.25
    for k in (-24, -21, -19, 6):
        got = query(ds, upload(rf.scaled(base_rays, k)), n, outputs=("hits",))["hits"]
        sel = np.ones(n, dtype=bool) if k < 0 else (~hit | (t0 > 0.25))
        differ = sel & (got[:, 0] != base[:, 0])
        assert not differ.any(), (k, int(differ.sum()), np.nonzero(differ)[0][:8], got[differ][:4], base[differ][:4])
        s = sel & hit
        t = np.ldexp(np.where(s, got[:, 1].copy().view(F), F(1.0)), k).astype(F)  # (a miss's t word holds no float)
        off = s & (t.view(np.int32) != t0.view(np.int32))
        assert not off.any(), (k, int(off.sum()), np.nonzero(off)[0][:8], t[off][:4], t0[off][:4])


@pytest.mark.parametrize("scene", ["wide", "mixed"])
@pytest.mark.parametrize("family", ["ao", "axis_occ"])
def test_scaled_directions_occlusion(scene, family):
    """d · 2^k with tmin · 2^-k and tmax · 2^-k: the same `occluded` bytes, on both sides of the switch at 2^+-40."""
    ds = device(scene)
    base_rays = rf.family_case(scene, family)["rays"]
    n = base_rays.shape[0]
    base = occluded(ds, upload(base_rays), n, outputs=("occluded",))["occluded"]
    assert 0 < base.mean() < 1
    for k in (-24, -21, -19, 19, 21):
        got = occluded(ds, upload(rf.scaled(base_rays, k, ranges=True)), n, outputs=("occluded",))["occluded"]
        differ = got != base
        assert not differ.any(), (k, int(differ.sum()), np.nonzero(differ)[0][:8])


# ---------------------------------------------------------------------------------------------------------------------
# d. Schedule
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scene", ["wide", "rects"])
@pytest.mark.parametrize("family", rf.QUERY_FAMILIES + rf.OCCLUSION_FAMILIES)
def test_schedule(scene, family):
    """One ray per lane and sixteen (a lane that finishes takes the wave's next ray, out of order): the same bits in
    every output, guards untouched (checked by the wrappers)."""
    ds = device(scene)
    rays = upload(rf.family_case(scene, family)["rays"])
    n = rays.shape[0]
    if family in rf.QUERY_FAMILIES:
        same_bits(query(ds, rays, n, rays_per_lane=1), query(ds, rays, n, rays_per_lane=16))
    else:
        same_occlusion_bits(occluded(ds, rays, n, rays_per_lane=1), occluded(ds, rays, n, rays_per_lane=16))
