"""The ray families of tests/ray_families.py without a device: what tests/test_gpu_ray_families.py relies on, asserted
on the brute-force reference alone.

Every (scene, family) keeps its undecidable share under the project's cap, shows the outcomes it is there for and makes
the reference compute no NaN t.  On the scene with 32-bit BVH references the hits reach BVH indices of 8192 and above.
Scaling a direction by a power of two changes nothing in the reference but the unit of t: the property the GPU test
asserts of the kernels bit for bit.  And the one ray the header leaves unspecified — a ray lying in a rectangle's plane
— is pinned as the oracle answers it: accepted, with t = NaN, whatever the rectangle's extent."""
from __future__ import annotations

import ctypes as C

import numpy as np
import pytest

from oracle import py_oracle as po

import ray_families as rf
from test_denoise_host import FLT_MAX, UNDECIDABLE_CAP, closest_hits
from test_occlusion_host import hittable_hits, occlusion_reference, one_primitive_scene
from test_query_host import uv_spread

F = np.float32
CASES = [(s, f) for s in rf.SCENES for f in rf.QUERY_FAMILIES + rf.OCCLUSION_FAMILIES]


@pytest.mark.parametrize("scene,family", CASES)
def test_family_reference(scene, family):
    """The cap (a condition, not a measurement), both outcomes, no NaN t, and the family's own shape."""
    case = rf.family_case(scene, family)
    rays = case["rays"]
    n = rays.shape[0]
    assert n <= 960 and rays.dtype == F and np.isfinite(rays[:, :, :3]).all()
    share = 1.0 - float(case["decidable"].mean())
    assert not rf.in_plane(rf.scene(scene), rays).any()
    if family in rf.QUERY_FAMILIES:
        positive = case["prim_id"] >= 0
        assert not np.isnan(case["normal_depth"]).any() and not np.isnan(case["uv"]).any()
        assert np.all(case["normal_depth"][positive, 3] > 0.001)
        print(f"{scene} {family}: undecidable {share:.4f}, hits {positive.mean():.3f}, uv spread {uv_spread(case):.2e}")
    else:
        positive = case["occluded"]
        by_radius = [round(float(positive[i::3].mean()), 3) for i in range(3)] if family == "ao" else ""
        print(f"{scene} {family}: undecidable {share:.4f}, occluded {positive.mean():.3f} {by_radius}")
    assert share <= UNDECIDABLE_CAP, share
    dec = case["decidable"]
    assert (positive & dec).any() and (~positive & dec).any()
    if family in ("interior", "ao"):
        assert 0.05 <= positive.mean() <= 0.95, positive.mean()
    d = rays[:, 1, :3]
    zeros = (d == 0).sum(1)
    if family in ("axis", "axis_occ"):
        assert np.all(zeros == 2) and np.all(np.abs(d).max(1) == 1.0)
        odd = np.arange(n) % 2 == 1
        assert np.all(np.signbit(d[odd][d[odd] == 0])) and not np.signbit(d[~odd][d[~odd] == 0]).any()
        for k, (ax, sign) in enumerate(rf.AXES):  # all six signed axes, 160 rays each, from outside the populated box
            s = slice(160 * k, 160 * (k + 1))
            assert np.all(d[s, ax] == sign)
            lo, hi = rf.BOXES[scene]
            assert np.all(rays[s, 0, ax] < lo[ax]) if sign > 0 else np.all(rays[s, 0, ax] > hi[ax])
    elif family == "planar":
        assert np.all(zeros == 1)
        z = d[d == 0]
        assert np.signbit(z).any() and not np.signbit(z).all()
        assert len(np.unique(np.round(np.linalg.norm(d, axis=1), 4))) >= 4  # not normalised
    elif family == "tiny":
        assert np.all(zeros == 1) and np.all(np.abs(d).min(1) == 0) and np.all(np.sort(np.abs(d), 1)[:, 1] == F(2.0 ** -130))
    else:
        assert np.all(zeros == 0)
    if family == "ao":
        assert np.all(rays[:, 0, 3] == F(0.001)) and sorted(set(rays[:, 1, 3].tolist())) == [0.25, 1.0, 4.0]
    if family == "axis_occ":
        assert np.all(rays[:, 0, 3] == F(0.001)) and np.all(np.isposinf(rays[:, 1, 3]))


def test_swapping_the_zero_signs_keeps_the_reference():
    """-0 on the even indices in place of the odd ones: the same primitive for every axis ray (what the GPU test asserts
    of the kernels, bit for bit)."""
    for scene in ("rects", "mixed"):
        a, b = rf.axis(scene), rf.axis(scene, neg_zero="even")
        assert np.array_equal(a, b) and a.tobytes() != b.tobytes()  # equal as numbers, not as bits
        sc = rf.scene(scene)
        ids = closest_hits(sc, b[:, 0, :3], b[:, 1, :3])[0]
        assert np.array_equal(ids, rf.family_case(scene, "axis")["prim_id"])


@pytest.mark.parametrize("family", ["axis", "interior"])
def test_wide_hits_reach_the_upper_reference_bits(family):
    sc = rf.scene("wide")
    src = rf.prim_source(sc)
    bvh_index = np.argsort(src)  # hittable index -> index in BVH order (every hittable is active)
    assert np.array_equal(src[bvh_index], np.arange(len(src)))
    case = rf.family_case("wide", family)
    ids = case["prim_id"][case["decidable"] & (case["prim_id"] >= 0)]
    top = int(bvh_index[ids].max())
    print(f"wide {family}: largest BVH index among the decidable hits {top}")
    assert top >= 8192, top


@pytest.mark.parametrize("family", ["axis", "interior"])
def test_scaling_property_of_the_reference(family):
    """d * 2^k: the same primitive on every ray and t * 2^k the unscaled t bit for bit, for the scales on both sides of
    the kernels' switch at dot(d, d) = 2^-40.  k = +6: only rays whose unscaled t exceeds 0.25 and the misses (the
    fixed tmin of 0.001 is 0.064 in the unscaled ray's units there)."""
    sc = rf.scene("wide")
    case = rf.family_case("wide", family)
    o, d = np.ascontiguousarray(case["rays"][:, 0, :3]), np.ascontiguousarray(case["rays"][:, 1, :3])
    ids0, t0 = case["prim_id"], case["normal_depth"][:, 3]
    hit = ids0 >= 0
    for k in (-24, -21, -19, 6):
        dk = np.ldexp(d, k)
        assert np.array_equal(np.ldexp(dk, -k), d)  # exact
        ids, recs = closest_hits(sc, o, dk, records=True, prefilter_d=d)
        sel = np.ones(len(ids0), dtype=bool) if k < 0 else (~hit | (t0 > 0.25))
        assert sel.sum() > 0.6 * len(sel)
        assert np.array_equal(ids[sel], ids0[sel]), (k, np.nonzero(sel & (ids != ids0))[0][:8])
        t = np.array([recs[r].t if ids[r] >= 0 else -1.0 for r in range(len(ids))], dtype=F)
        rescaled = np.where(ids >= 0, np.ldexp(t, k), F(-1.0)).astype(F)
        assert rescaled[sel].tobytes() == t0[sel].tobytes(), k


def test_scaled_rays_are_exact():
    rays = rf.family_case("rects", "ao")["rays"]
    for k in (-24, 19, 21):
        s = rf.scaled(rays, k, ranges=True)
        assert np.array_equal(np.ldexp(s[:, 1, :3], -k), rays[:, 1, :3])
        assert np.array_equal(np.ldexp(s[:, 0, 3], k), rays[:, 0, 3]) and np.array_equal(np.ldexp(s[:, 1, 3], k), rays[:, 1, 3])
        assert np.array_equal(s[:, 0, :3], rays[:, 0, :3])
    inf = rf.scaled(rf.axis_occ("rects"), -24, ranges=True)
    assert np.all(np.isposinf(inf[:, 1, 3])) and np.all(inf[:, 0, 3] == np.ldexp(F(0.001), 24))


def test_a_ray_in_a_rectangles_plane_is_accepted_with_a_nan_t():
    """include/rt_hip.h leaves this ray's result unspecified, and this is why: the reference's rectangle test computes
    t = (k - o_k) * (1 / d_k) = 0 * inf = NaN, which fails none of its comparisons — the ray "hits" the 2 x 2 rectangle
    from 50 units outside its extent.  No BVH kernel can agree (the rectangle's box is nowhere near the ray), and every
    family asserts that it holds no such ray (in_plane)."""
    sc = one_primitive_scene("rect")
    h = sc.hittables[0]
    o, d = np.array([50.0, 50.0, -1.0], dtype=F), np.array([1.0, 0.0, 0.0], dtype=F)
    assert hittable_hits(h, o, d, 0.001, FLT_MAX)
    rec = po.Hit()
    fp = C.POINTER(C.c_float)
    assert po.lib().orc_hittable_hit(C.byref(h), o.ctypes.data_as(fp), d.ctypes.data_as(fp), F(0.001), F(FLT_MAX), C.byref(rec))
    assert np.isnan(rec.t)
    rays = np.zeros((3, 2, 4), dtype=F)
    rays[:, 0, :3], rays[:, 1, :3] = o, d
    rays[1, 1, 2] = -0.0              # -0: the same
    rays[2, 0, 2] = np.nextafter(F(-1.0), F(0.0))  # one float off the plane: t = +inf, rejected
    rays[:, 0, 3], rays[:, 1, 3] = 0.001, FLT_MAX
    assert rf.in_plane(sc, rays).tolist() == [True, True, False]
    assert occlusion_reference(sc, rays, prefilter=False).tolist() == [True, True, False]
    # off the plane the ray is fully specified, zero components and all, also over a range that ends at +inf
    rays[:, 1, 3] = np.inf
    assert occlusion_reference(sc, rays, prefilter=False).tolist() == [True, True, False]
