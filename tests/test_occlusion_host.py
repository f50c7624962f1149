"""rt_occluded_rays without a device: the struct against the header, the export, every argument check, and the
reference that tests/test_gpu_occlusion.py compares the kernel with.

occlusion_reference restates the call's definition: a ray with !(tmin <= tmax) is unoccluded; any other ray is occluded
exactly when some active hittable's own test — the oracle's orc_hittable_hit(h, o, d, tmin, tmax) — accepts.
shadow_case builds the shadow rays of a query frame (tests/test_query_host.py, query_case): from every hit point
P = o + t·d towards the point light L = (2, 5, 3) with d = L − P and the range (0.001, 1), the camera's misses left as
they are with (0.001, FLT_MAX).  A ray is decidable when the closest-hit frame's own rule holds for its pixel and the
reference answers the same for seven nearby questions: L as given, L shifted by ±1/256 in x and in z, and tmin 0.0005
and 0.002 in place of 0.001 — a ray that grazes a silhouette, or whose origin sits on the surface it would hit, fails
one of them."""
from __future__ import annotations

import ctypes as C
import functools
import os
import re

import numpy as np
import pytest

from cudaraytracer_amd import abi, scenes
from cudaraytracer_amd._lib import EXPORTED, lib
from oracle import py_oracle as po

from test_denoise_host import FLT_MAX, UNDECIDABLE_CAP, _candidates
from test_query_host import query_case, query_scene

F = np.float32
HEADER = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "rt_hip.h")).read()
LIGHT = (2.0, 5.0, 3.0)
# the frames of the reference tests: (scene, camera, size)
SHADOW_FRAMES = (("rtiow", "near", (40, 24)), ("rtiow", "near", (37, 21)), ("wide", "near", (37, 21)),
                 ("wide", "far", (37, 21)))


# ---------------------------------------------------------------------------------------------------------------------
# The reference
# ---------------------------------------------------------------------------------------------------------------------
def hittable_hits(h: abi.HittableDesc, o: np.ndarray, d: np.ndarray, tmin, tmax) -> bool:
    """The oracle's own test of one hittable over [tmin, tmax] on float32 inputs."""
    fp = C.POINTER(C.c_float)
    o, d = np.ascontiguousarray(o, dtype=F), np.ascontiguousarray(d, dtype=F)
    rec = po.Hit()
    return bool(po.lib().orc_hittable_hit(C.byref(h), o.ctypes.data_as(fp), d.ctypes.data_as(fp), F(tmin), F(tmax), C.byref(rec)))


def occlusion_reference(scene, rays: np.ndarray, prefilter: bool = True) -> np.ndarray:
    """occluded (n,) bool of rays (n, 2, 4) float32.  prefilter: test only _candidates' superset (built for t above
    about -1: off for ranges that reach further back)."""
    rays = np.ascontiguousarray(rays, dtype=F)
    o, d = np.ascontiguousarray(rays[:, 0, :3]), np.ascontiguousarray(rays[:, 1, :3])
    tmin, tmax = rays[:, 0, 3], rays[:, 1, 3]
    with np.errstate(invalid="ignore"):
        valid = tmin <= tmax  # (false with a NaN at either end)
    active = np.array([bool(h.is_active) for h in scene.hittables], dtype=bool)
    cand = _candidates(scene, o, d) if prefilter else np.broadcast_to(active, (rays.shape[0], len(active)))
    L = po.lib()
    fp = C.POINTER(C.c_float)
    out = np.zeros(rays.shape[0], dtype=bool)
    rec = po.Hit()
    for r in np.nonzero(valid & cand.any(1))[0]:
        op, dp = o[r].ctypes.data_as(fp), d[r].ctypes.data_as(fp)
        for i in np.nonzero(cand[r])[0]:
            if L.orc_hittable_hit(C.byref(scene.hittables[int(i)]), op, dp, tmin[r], tmax[r], C.byref(rec)):
                out[r] = True
                break
    return out


def shadow_rays(ref: dict, light=LIGHT, tmin: float = 0.001) -> np.ndarray:
    """The shadow rays (n, 2, 4) of a query frame's reference: float32 arithmetic throughout."""
    o, d = ref["rays"][:, 0, :3], ref["rays"][:, 1, :3]
    hit = ref["prim_id"] >= 0
    t = ref["normal_depth"][:, 3]
    p = (o + t[:, None] * d).astype(F)
    rays = np.zeros_like(ref["rays"])
    rays[:, 0, :3] = np.where(hit[:, None], p, o)
    rays[:, 1, :3] = np.where(hit[:, None], np.array(light, dtype=F)[None, :] - p, d)
    rays[:, 0, 3] = F(tmin)
    rays[:, 1, 3] = np.where(hit, F(1.0), F(FLT_MAX))
    return rays


def shadow_reference(scene, ref: dict) -> dict:
    rays = shadow_rays(ref)
    occluded = occlusion_reference(scene, rays)
    decidable = ref["decidable"].copy()
    e = 1.0 / 256.0
    lx, ly, lz = LIGHT
    for light, tmin in (((lx + e, ly, lz), 0.001), ((lx - e, ly, lz), 0.001), ((lx, ly, lz + e), 0.001),
                        ((lx, ly, lz - e), 0.001), (LIGHT, 0.0005), (LIGHT, 0.002)):
        decidable &= occlusion_reference(scene, shadow_rays(ref, light, tmin)) == occluded
    out = {"rays": rays, "occluded": occluded, "decidable": decidable, "camera_hit": ref["prim_id"] >= 0}
    for a in out.values():
        a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def shadow_case(scene: str, camera: str, size: tuple) -> dict:
    """One frame's shadow rays and their reference, computed once per process and shared (read-only)."""
    return shadow_reference(query_scene(scene), query_case(scene, camera, size))


def one_primitive_scene(kind: str) -> scenes.Scene:
    """"rect": an XY rectangle of 2 x 2 at z = -1; "sphere": a sphere of radius 1 at (0, 0, -3)."""
    h = (abi.HittableDesc * 1)()
    m = (abi.MaterialDesc * 1)()
    m[0].type, m[0].albedo.type, m[0].albedo.image = abi.RT_LAMBERTIAN, abi.RT_CONSTANT, -1
    m[0].albedo.color[:] = [0.5, 0.5, 0.5]
    h[0].is_active, h[0].material = 1, 0
    if kind == "rect":
        h[0].type, h[0].width, h[0].height = abi.RT_XYRECT, 2.0, 2.0
        h[0].center[:] = [0.0, 0.0, -1.0]
    else:
        h[0].type, h[0].radius = abi.RT_SPHERE, 1.0
        h[0].center[:] = [0.0, 0.0, -3.0]
    return scenes.Scene(h, m, [])


def _up(x, towards):
    return float(np.nextafter(F(x), F(towards)))


E = 2.0 ** -10
NAN = float("nan")
# From the origin along (0, 0, -1): the rectangle is met at t = 1 exactly, the sphere's roots are 2 and 4 exactly.
# (tmin, tmax, occluded)
HAND_RANGES = {
    "rect": ((1.0, 1.0, 1), (1.0, 2.0, 1), (0.5, 1.0, 1),           # closed at both ends
             (0.5, _up(1, 0), 0), (_up(1, 2), 2.0, 0),               # one float short of / past t
             (0.0, FLT_MAX, 1), (-3.0, float("inf"), 1), (2.0, 9.0, 0),
             (2.0, 1.0, 0), (NAN, 2.0, 0), (0.5, NAN, 0), (NAN, NAN, 0)),
    "sphere": ((2.0 - E, 3.0, 1), (2.0 + E, 4.0 - E, 0),              # the near root; between the roots
               (2.0 + E, 4.0 + E, 1), (5.0, 9.0, 0),                  # the far root; behind the sphere
               (2.0, 4.0, 0), (2.0, _up(4, 5), 1), (_up(2, 0), 2.5, 1),  # open at both ends
               (0.0, FLT_MAX, 1), (-1.0, float("inf"), 1),
               (3.0, 2.5, 0), (NAN, 3.0, 0), (1.0, NAN, 0)),
}


def hand_rays(kind: str) -> tuple:
    """rays (k, 2, 4) float32 and the expected occluded (k,) of HAND_RANGES[kind]."""
    cases = HAND_RANGES[kind]
    rays = np.zeros((len(cases), 2, 4), dtype=F)
    rays[:, 1, 2] = -1.0
    rays[:, 0, 3] = [c[0] for c in cases]
    rays[:, 1, 3] = [c[1] for c in cases]
    return rays, np.array([c[2] for c in cases], dtype=bool)


@pytest.mark.parametrize("kind", ["rect", "sphere"])
def test_hand_made_ranges(kind):
    """The expected values are the oracle's own: orc_hittable_hit on the same float32 inputs, after the range rule."""
    scene = one_primitive_scene(kind)
    rays, expected = hand_rays(kind)
    for r, want in zip(rays, expected):
        tmin, tmax = r[0, 3], r[1, 3]
        own = bool(tmin <= tmax) and hittable_hits(scene.hittables[0], r[0, :3], r[1, :3], tmin, tmax)
        assert own == bool(want), (kind, float(tmin), float(tmax))
    assert np.array_equal(occlusion_reference(scene, rays, prefilter=False), expected)
    assert np.array_equal(occlusion_reference(scene, rays), expected)
    # a range behind the origin: the rectangle seen backwards at t = -1, the sphere's roots at -4 and -2
    back = rays[:3].copy()
    back[:, 1, 2] = 1.0
    back[:, 0, 3], back[:, 1, 3] = (-5.0, -1.0, -1.5), (-0.5, 5.0, -1.25)
    want = {"rect": [True, True, False], "sphere": [True, False, False]}[kind]
    assert occlusion_reference(scene, back, prefilter=False).tolist() == want


def test_reference_ignores_inactive_hittables_and_empty_scenes():
    rays, _ = hand_rays("sphere")
    s = one_primitive_scene("sphere")
    s.hittables[0].is_active = 0
    assert not occlusion_reference(s, rays).any() and not occlusion_reference(s, rays, prefilter=False).any()


@pytest.mark.parametrize("scene,camera,size", SHADOW_FRAMES)
def test_shadow_frames(scene, camera, size):
    """The undecidable share of every frame of the GPU test is under the project's cap, on the reference alone; both
    answers occur among the decidable rays."""
    case = shadow_case(scene, camera, size)
    share = 1.0 - float(case["decidable"].mean())
    hit = case["camera_hit"]
    occ = float(case["occluded"][hit].mean())
    print(f"{scene} {camera} {size[0]}x{size[1]}: undecidable {share:.4f}, occluded hit rays {occ:.3f}, misses {(~hit).mean():.3f}")
    assert share <= UNDECIDABLE_CAP, share
    dec = case["decidable"]
    assert (case["occluded"] & dec).sum() > 50 and (~case["occluded"] & dec & hit).sum() > 20
    assert not case["occluded"][~hit].any()  # (a camera ray that missed with (0.001, FLT_MAX) is unoccluded over it)
    assert np.all(case["rays"][hit, 1, 3] == 1.0) and np.all(case["rays"][~hit, 1, 3] == F(FLT_MAX))
    if camera == "far":
        assert (~hit).mean() > 0.25


# ---------------------------------------------------------------------------------------------------------------------
# The C ABI
# ---------------------------------------------------------------------------------------------------------------------
def test_struct_matches_the_header():
    """rt_occlusion_args: four pointers, four uint32 and reserved[2], in the header's order."""
    m = re.search(r"typedef struct rt_occlusion_args \{(.*?)\} rt_occlusion_args;", HEADER, re.S)
    assert m
    body = re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S)
    decls = [decl.strip() for decl in body.split(";") if decl.strip()]
    names = [re.sub(r"[\s*]|\[\d+\]", "", decl.split()[-1]) for decl in decls]
    assert names == [f[0] for f in abi.OcclusionArgs._fields_]
    assert names == ["rays", "occluded", "blocker", "counters", "n", "rays_per_lane", "count_tests", "flags", "reserved"]
    assert decls[-1].endswith("reserved[2]") and decls[-1].startswith("uint32_t")
    assert C.sizeof(abi.OcclusionArgs) == 4 * 8 + 6 * 4
    for i, name in enumerate(names[:4]):
        assert "*" in decls[i] and getattr(abi.OcclusionArgs, name).offset == 8 * i
    for i, name in enumerate(names[4:]):
        assert decls[4 + i].startswith("uint32_t") and getattr(abi.OcclusionArgs, name).offset == 32 + 4 * i
    assert abi.OcclusionArgs.reserved.size == 8


def test_export_and_abi_version():
    assert "rt_occluded_rays" in EXPORTED
    assert hasattr(lib(), "rt_occluded_rays")
    assert lib().rt_abi_version() == 14 and abi.ABI_VERSION == 14  # (an addition that changes no layout)
    assert "#define RT_ABI_VERSION 14" in HEADER
    # the header's list of additions that keep the number names it
    comment = HEADER[:HEADER.index("#define RT_ABI_VERSION")]
    assert "rt_occluded_rays" in comment[comment.rindex("/*"):]


def _args(n: int = 64):
    """Valid arguments over host dummies (never dereferenced: every check precedes the first device call)."""
    bufs = {"rays": C.create_string_buffer(max(1, n) * 32), "occluded": C.create_string_buffer(max(1, n)),
            "blocker": C.create_string_buffer(max(1, n) * 4), "counters": C.create_string_buffer(abi.COUNTERS_WORDS * 8)}
    a = abi.OcclusionArgs()
    for name, b in bufs.items():
        setattr(a, name, C.addressof(b))
    a.n = n
    return a, bufs


def _rejected(rc: int, what: str | None = None) -> None:
    assert rc == -1, rc
    msg = lib().rt_last_error()
    assert b"rt_occluded_rays" in msg, msg
    if what:
        assert what.encode() in msg, msg


OUTPUTS = (("occluded", 1 * 64), ("blocker", 4 * 64), ("counters", abi.COUNTERS_WORDS * 8))  # name, bytes at n = 64


def test_rejects_bad_arguments():
    L = lib()
    scene = C.cast(C.create_string_buffer(64), C.c_void_p)  # never dereferenced: the arguments are checked first
    _rejected(L.rt_occluded_rays(scene, None, None), "NULL args")
    a, keep = _args()
    _rejected(L.rt_occluded_rays(None, C.byref(a), None), "NULL scene")
    a, keep = _args()
    a.rays = None
    _rejected(L.rt_occluded_rays(scene, C.byref(a), None), "NULL rays")
    a, keep = _args()
    a.occluded = a.blocker = None
    _rejected(L.rt_occluded_rays(scene, C.byref(a), None), "no output")
    for bad in (2, 3, 1 << 31, 0xffffffff):
        a, keep = _args()
        a.count_tests = bad
        _rejected(L.rt_occluded_rays(scene, C.byref(a), None), "count_tests")
    a, keep = _args()
    a.count_tests, a.counters = 1, None
    _rejected(L.rt_occluded_rays(scene, C.byref(a), None), "without counters")
    for bad in (17, 64, 0xffffffff):
        a, keep = _args()
        a.rays_per_lane = bad
        _rejected(L.rt_occluded_rays(scene, C.byref(a), None), "rays_per_lane")
    for bad in (1, 1 << 31):
        a, keep = _args()
        a.flags = bad
        _rejected(L.rt_occluded_rays(scene, C.byref(a), None), "flags")
        for k in (0, 1):
            a, keep = _args()
            a.reserved[k] = bad
            _rejected(L.rt_occluded_rays(scene, C.byref(a), None), "reserved")
    # each output alone, count_tests = 1 with counters, 16 rays per lane: valid (a NULL scene stops the call)
    for only in ("occluded", "blocker"):
        a, keep = _args()
        setattr(a, "blocker" if only == "occluded" else "occluded", None)
        a.count_tests, a.rays_per_lane = 1, 16
        _rejected(L.rt_occluded_rays(None, C.byref(a), None), "NULL scene")


def test_rejects_overlapping_buffers():
    """An output, counters included, may share no byte with `rays` or with another output."""
    L = lib()
    scene = C.cast(C.create_string_buffer(64), C.c_void_p)
    for name, _ in OUTPUTS:
        a, keep = _args()
        setattr(a, name, a.rays)
        _rejected(L.rt_occluded_rays(scene, C.byref(a), None), "overlaps rays")
        a, keep = _args()
        setattr(a, name, a.rays + 64 * 32 - 1)  # the last byte of the rays
        _rejected(L.rt_occluded_rays(scene, C.byref(a), None), "overlaps rays")
    for i, (first, nbytes) in enumerate(OUTPUTS):
        for second, _ in OUTPUTS[i + 1:]:
            a, keep = _args()
            setattr(a, second, getattr(a, first))
            _rejected(L.rt_occluded_rays(scene, C.byref(a), None), "overlap")
            a, keep = _args()
            setattr(a, second, getattr(a, first) + nbytes - 1)  # the second's first byte is the first's last
            _rejected(L.rt_occluded_rays(scene, C.byref(a), None), "overlap")
    a, keep = _args()
    a.occluded = a.blocker + 64 * 4  # adjacent, not overlapping: passes the argument checks (a NULL scene stops it)
    _rejected(L.rt_occluded_rays(None, C.byref(a), None), "NULL scene")


def test_no_rays_is_accepted_without_a_device():
    a, keep = _args(0)
    assert lib().rt_occluded_rays(None, C.byref(a), None) == 0
    a.rays = None
    assert lib().rt_occluded_rays(None, C.byref(a), None) == 0
    # ... but the arguments are still checked
    a.flags = 1
    _rejected(lib().rt_occluded_rays(None, C.byref(a), None), "flags")
    a.flags, a.count_tests = 0, 2
    _rejected(lib().rt_occluded_rays(None, C.byref(a), None), "count_tests")
