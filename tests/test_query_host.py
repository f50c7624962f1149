"""rt_query_rays without a device: the struct against the header, the export and ABI 14, every argument check, and the
numpy reference of the per-ray record that tests/test_gpu_query.py compares the kernel with.

query_reference restates rt_query_rays' outputs for a frame of camera centre rays (camera_rays of
tests/test_denoise_host.py with both jitter numbers 0.5, handed to the kernel as they are): the brute-force closest hit
through the oracle's primitive tests (closest_hits(..., records=True)), the record's normal and t, the albedo as
gbuffer_reference derives it (a miss gets (0, 0, 0, 0): no camera, no sky), and — beyond rt_gbuffer's planes — the
surface's (u, v) for every sphere and rectangle and the hittable's material index.  `uv64` is the same (u, v) in float64
from the float64 hit point; the spread between the two is what the GPU test's uv bound is built from.  `decidable` is
gbuffer_reference's rule: the centre ray and the four rays shifted by +-1/64 pixel hit the same primitive.
records_reference is the same derivation for any rays and any set of nearby rays (tests/ray_families.py)."""
from __future__ import annotations

import ctypes as C
import functools
import os
import re

import numpy as np
import pytest

from cudaraytracer_amd import abi, scenes
from cudaraytracer_amd._lib import EXPORTED, lib

from test_denoise_host import UNDECIDABLE_CAP, _texture_value, camera_rays, closest_hits

F = np.float32
HEADER = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "rt_hip.h")).read()

QUERY_SIZES = ((40, 24), (37, 21))


def query_cameras() -> dict:
    """The two 20-degree cameras of the query tests; "far" sees 46 % sky and supplies the misses."""
    return {"near": scenes.camera_inputs((3.0, 1.0, 1.0), scenes.normalized((-3.0, -0.6, -1.0)), 20.0),
            "far": scenes.camera_inputs((13.0, 2.0, 3.0), scenes.normalized((-13.0, 1.5, -3.0)), 20.0)}


@functools.lru_cache(maxsize=None)
def query_scene(name: str) -> scenes.Scene:
    """"rtiow": the built-in RTIOW scene (16-bit references); "wide": sphere_field(9000, 6) (32-bit references)."""
    return {"rtiow": lambda: scenes.builtin(scenes.SCENE_RTIOW), "wide": lambda: scenes.sphere_field(9000, 6)}[name]()


def uv_float64(h: abi.HittableDesc, o: np.ndarray, d: np.ndarray) -> tuple:
    """(u, v) of the closest intersection of the ray with hittable `h` in float64 (the ray's float32 values widened)."""
    o, d = o.astype(np.float64), d.astype(np.float64)
    c = np.array(h.center[:], dtype=np.float64)
    if h.type == abi.RT_SPHERE:
        oc = o - c
        a, hb, cc = d @ d, oc @ d, oc @ oc - float(h.radius) ** 2
        root = np.sqrt(max(hb * hb - a * cc, 0.0))
        t = (-hb - root) / a
        if not 0.001 < t:
            t = (-hb + root) / a
        n = (o + t * d - c) / float(h.radius)
        return (np.arctan2(-n[2], n[0]) + np.pi) / (2.0 * np.pi), np.arccos(min(1.0, max(-1.0, -n[1]))) / np.pi
    ia, ib, ik, ea, eb = {abi.RT_XYRECT: (0, 1, 2, h.width, h.height), abi.RT_XZRECT: (0, 2, 1, h.width, h.height),
                          abi.RT_YZRECT: (1, 2, 0, h.height, h.width)}[h.type]
    t = (c[ik] - o[ik]) / d[ik]
    a0, b0 = float(F(c[ia]) - F(ea) / F(2)), float(F(c[ib]) - F(eb) / F(2))
    a1, b1 = float(F(c[ia]) + F(ea) / F(2)), float(F(c[ib]) + F(eb) / F(2))
    return (o[ia] + t * d[ia] - a0) / (a1 - a0), (o[ib] + t * d[ib] - b0) / (b1 - b0)


def records_reference(scene, o: np.ndarray, d: np.ndarray, shifts) -> dict:
    """rt_query_rays' outputs for the rays (o, d), each (n, 3) float32, by brute force over the description, and the rays
    themselves as (n, 2, 4) float32.  `shifts`: (o2, d2) pairs of nearby rays; a ray is decidable when every one of them
    hits the primitive the ray itself hits."""
    n = o.shape[0]
    ids, recs = closest_hits(scene, o, d, records=True)
    decidable = np.ones(n, dtype=bool)
    for o2, d2 in shifts:
        decidable &= closest_hits(scene, o2, d2)[0] == ids
    rays = np.zeros((n, 2, 4), dtype=F)
    rays[:, 0, :3], rays[:, 1, :3] = o, d
    nd = np.zeros((n, 4), dtype=F)
    alb = np.zeros((n, 4), dtype=F)
    uv = np.zeros((n, 2), dtype=F)
    uv64 = np.zeros((n, 2), dtype=np.float64)
    material = np.full(n, -1, dtype=np.int32)
    for r in range(n):
        if ids[r] < 0:
            nd[r] = (0.0, 0.0, 0.0, -1.0)
            continue
        rec, h = recs[r], scene.hittables[int(ids[r])]
        nd[r] = (rec.normal[0], rec.normal[1], rec.normal[2], rec.t)
        uv[r] = (rec.u, rec.v)
        uv64[r] = uv_float64(h, o[r], d[r])
        material[r] = h.material
        m = scene.materials[h.material]
        alb[r] = 1.0  # Dielectric: (1, 1, 1)
        if m.type != abi.RT_DIELECTRIC:
            tex = _texture_value(scene, m.albedo, rec.u, rec.v, rec.p)
            alb[r, :3] = F(m.light_intensity) * tex if m.type == abi.RT_DIFFUSELIGHT else tex
    out = {"rays": rays, "normal_depth": nd, "albedo": alb, "prim_id": ids, "uv": uv, "uv64": uv64, "material": material,
           "decidable": decidable}
    for a in out.values():
        a.setflags(write=False)
    return out


def query_reference(scene, inputs: abi.InputStruct, width: int, height: int) -> dict:
    """The rays (n, 2, 4) float32 of the frame's centre rays and rt_query_rays' outputs for them (n = width * height)."""
    o, d = camera_rays(inputs, width, height, 0.5, 0.5)
    e = 1.0 / 64.0
    shifts = []
    for sx, sy in ((e, 0.0), (-e, 0.0), (0.0, e), (0.0, -e)):
        o2, d2 = camera_rays(inputs, width, height, 0.5 + sx, 0.5 + sy)
        shifts.append((o2.reshape(-1, 3), d2.reshape(-1, 3)))
    return records_reference(scene, o.reshape(-1, 3), d.reshape(-1, 3), shifts)


@functools.lru_cache(maxsize=None)
def query_case(scene: str, camera: str, size: tuple) -> dict:
    """One frame's reference, computed once per process and shared (read-only)."""
    return query_reference(query_scene(scene), query_cameras()[camera], *size)


def uv_spread(ref: dict) -> float:
    """d: the largest float32-against-float64 difference of the reference's (u, v) over the decidable hits."""
    sel = ref["decidable"] & (ref["prim_id"] >= 0)
    return float(np.abs(ref["uv"][sel].astype(np.float64) - ref["uv64"][sel]).max()) if sel.any() else 0.0


# ---------------------------------------------------------------------------------------------------------------------
# The C ABI
# ---------------------------------------------------------------------------------------------------------------------
def test_struct_matches_the_header():
    """rt_query_args: seven pointers and four uint32, in the header's order."""
    m = re.search(r"typedef struct rt_query_args \{(.*?)\} rt_query_args;", HEADER, re.S)
    assert m
    body = re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S)
    names = [re.sub(r"[\s*]", "", decl.split()[-1]) for decl in body.split(";") if decl.strip()]
    assert names == [f[0] for f in abi.QueryArgs._fields_]
    assert C.sizeof(abi.QueryArgs) == 7 * 8 + 4 * 4
    for i, name in enumerate(names[:7]):
        assert getattr(abi.QueryArgs, name).offset == 8 * i
    for i, name in enumerate(names[7:]):
        assert getattr(abi.QueryArgs, name).offset == 56 + 4 * i
    assert names[7:] == ["n", "rays_per_lane", "flags", "reserved"]


def test_export_and_abi_version():
    assert "rt_query_rays" in EXPORTED
    assert hasattr(lib(), "rt_query_rays")
    assert lib().rt_abi_version() == 14 and abi.ABI_VERSION == 14
    assert "#define RT_ABI_VERSION 14" in HEADER


def _args(n: int = 64):
    """Valid arguments over host dummies (never dereferenced: every check precedes the first device call)."""
    bufs = {"rays": C.create_string_buffer(max(1, n) * 32)}
    for name, size in (("normal_depth", 16), ("albedo", 16), ("prim_id", 4), ("uv", 8), ("material", 4), ("hits", 8)):
        bufs[name] = C.create_string_buffer(max(1, n) * size)
    a = abi.QueryArgs()
    for name, b in bufs.items():
        setattr(a, name, C.addressof(b))
    a.n = n
    return a, bufs


def _rejected(rc: int, what: str | None = None) -> None:
    assert rc == -1, rc
    msg = lib().rt_last_error()
    assert b"rt_query_rays" in msg, msg
    if what:
        assert what.encode() in msg, msg


OUTPUTS = ("normal_depth", "albedo", "prim_id", "uv", "material", "hits")


def test_rejects_bad_arguments():
    L = lib()
    scene = C.cast(C.create_string_buffer(64), C.c_void_p)  # never dereferenced: the arguments are checked first
    _rejected(L.rt_query_rays(scene, None, None), "NULL args")
    a, keep = _args()
    a.rays = None
    _rejected(L.rt_query_rays(scene, C.byref(a), None), "NULL rays")
    a, keep = _args()
    for name in OUTPUTS:
        setattr(a, name, None)
    _rejected(L.rt_query_rays(scene, C.byref(a), None), "no output")
    for bad in (17, 64, 0xffffffff):
        a, keep = _args()
        a.rays_per_lane = bad
        _rejected(L.rt_query_rays(scene, C.byref(a), None), "rays_per_lane")
    for field in ("flags", "reserved"):
        for bad in (1, 1 << 31):
            a, keep = _args()
            setattr(a, field, bad)
            _rejected(L.rt_query_rays(scene, C.byref(a), None), field)
    a, keep = _args()
    _rejected(L.rt_query_rays(None, C.byref(a), None), "NULL scene")


def test_rejects_overlapping_buffers():
    """An output may share no byte with `rays` or with another output: whole aliases and partial overlaps."""
    L = lib()
    scene = C.cast(C.create_string_buffer(64), C.c_void_p)
    for name in OUTPUTS:
        a, keep = _args()
        setattr(a, name, a.rays)
        _rejected(L.rt_query_rays(scene, C.byref(a), None), "overlaps rays")
        a, keep = _args()
        setattr(a, name, a.rays + 64 * 32 - 4)  # the last four bytes of the rays
        _rejected(L.rt_query_rays(scene, C.byref(a), None), "overlaps rays")
    for i, first in enumerate(OUTPUTS):
        for second in OUTPUTS[i + 1:]:
            a, keep = _args()
            setattr(a, second, getattr(a, first))
            _rejected(L.rt_query_rays(scene, C.byref(a), None), "overlap")
    a, keep = _args()
    a.prim_id = a.normal_depth + 64 * 16 - 4  # prim_id's first element is normal_depth's last word
    _rejected(L.rt_query_rays(scene, C.byref(a), None), "overlap")
    a, keep = _args()
    a.prim_id = a.normal_depth + 64 * 16  # adjacent, not overlapping: passes the argument checks (a NULL scene stops it)
    _rejected(L.rt_query_rays(None, C.byref(a), None), "NULL scene")


def test_no_rays_is_accepted_without_a_device():
    a, keep = _args(0)
    assert lib().rt_query_rays(None, C.byref(a), None) == 0
    a.rays = None
    assert lib().rt_query_rays(None, C.byref(a), None) == 0
    # ... but the arguments are still checked
    a.flags = 1
    _rejected(lib().rt_query_rays(None, C.byref(a), None), "flags")


# ---------------------------------------------------------------------------------------------------------------------
# The reference
# ---------------------------------------------------------------------------------------------------------------------
def test_reference_record_of_given_hits():
    """The record for hits known in closed form: rays down the axes onto a unit sphere and onto a rectangle."""
    h = (abi.HittableDesc * 2)()
    m = (abi.MaterialDesc * 2)()
    for k, (ty, col) in enumerate(((abi.RT_LAMBERTIAN, (0.2, 0.4, 0.6)), (abi.RT_DIFFUSELIGHT, (0.5, 0.25, 1.0)))):
        m[k].type, m[k].light_intensity = ty, 4
        m[k].albedo.type, m[k].albedo.image = abi.RT_CONSTANT, -1
        m[k].albedo.color[:] = list(col)
    h[0].type, h[0].is_active, h[0].material, h[0].radius = abi.RT_SPHERE, 1, 0, 1.0
    h[0].center[:] = [0.0, 0.0, 0.0]
    h[1].type, h[1].is_active, h[1].material, h[1].width, h[1].height = abi.RT_XZRECT, 1, 1, 4.0, 2.0
    h[1].center[:] = [10.0, -3.0, 0.0]
    scene = scenes.Scene(h, m, [])
    o = np.array([[3, 0, 0], [0, 0, 3], [11, -1, 0.5], [0, 5, 0], [20, 20, 20]], dtype=F)
    d = np.array([[-1, 0, 0], [0, 0, -2], [0, -1, 0], [0, -1, 0], [0, 1, 0]], dtype=F)
    ids, recs = closest_hits(scene, o, d, records=True)
    assert ids.tolist() == [0, 0, 1, 0, -1]
    # +x pole of the sphere: phi = atan2(-0, 1) + pi, theta = acos(-0)
    assert recs[0].t == 2.0 and tuple(recs[0].normal) == (1.0, 0.0, 0.0)
    assert abs(recs[0].u - 0.5) < 1e-6 and abs(recs[0].v - 0.5) < 1e-6
    # +z: phi = atan2(-1, 0) + pi = pi / 2; t in units of |direction| = 2
    assert recs[1].t == 1.0 and abs(recs[1].u - 0.25) < 1e-6 and abs(recs[1].v - 0.5) < 1e-6
    # the rectangle spans x in [8, 12], z in [-1, 1]; hit from above: the face normal points up
    assert recs[2].t == 2.0 and tuple(recs[2].normal) == (0.0, 1.0, 0.0)
    assert abs(recs[2].u - 0.75) < 1e-6 and abs(recs[2].v - 0.75) < 1e-6
    # the sphere's top: theta = acos(-1) = pi
    assert abs(recs[3].v - 1.0) < 1e-6
    for r in range(4):
        u64, v64 = uv_float64(scene.hittables[int(ids[r])], o[r], d[r])
        assert abs(u64 - recs[r].u) < 1e-6 and abs(v64 - recs[r].v) < 1e-6, (r, u64, v64, recs[r].u, recs[r].v)


@pytest.mark.parametrize("scene", ["rtiow", "wide"])
@pytest.mark.parametrize("camera", ["near", "far"])
@pytest.mark.parametrize("size", QUERY_SIZES)
def test_reference_frames(scene, camera, size):
    """Every frame of the GPU test: the undecidable share under the cap, hits present (misses under the far
    camera), the material of each hit the description's, and a (u, v) whose float32 and float64 values agree closely
    enough for 4 · d to be a bound worth asserting."""
    ref = query_case(scene, camera, size)
    share = 1.0 - float(ref["decidable"].mean())
    hit = ref["prim_id"] >= 0
    d = uv_spread(ref)
    print(f"{scene} {camera} {size[0]}x{size[1]}: undecidable {share:.4f}, hits {hit.mean():.3f}, uv spread d {d:.3e}")
    assert share <= UNDECIDABLE_CAP, share
    if camera == "far":  # (it looks over RTIOW's spheres: that frame is all sky; the sphere field reaches into it)
        assert (~hit).mean() > 0.25
    if (scene, camera) != ("rtiow", "far"):
        assert hit.mean() > 0.25
    hs = query_scene(scene).hittables
    assert all(ref["material"][r] == hs[int(ref["prim_id"][r])].material for r in np.nonzero(hit)[0])
    assert np.all(ref["material"][~hit] == -1) and not ref["uv"][~hit].any() and not ref["albedo"][~hit].any()
    assert np.all((ref["uv"][hit] >= 0) & (ref["uv"][hit] <= 1))
    # (largest where rays graze the 1000-unit ground sphere near its pole, where acos and atan2 are ill-conditioned; a ray
    # on atan2's seam would show as d near 1 and make the bound empty: none of these frames has one)
    assert d < 1e-2 and (d > 0 or not hit.any()), d
