"""Rays of the caller's own for rt_trace_rays / rt_query_rays / rt_occluded_rays, and their brute-force references.

The query and occlusion tests' other rays are the centre rays of 20-degree cameras and shadow rays towards one point
light.  The families here are what those leave out: rays with zero direction components (+0 and -0) on BVH scenes, waves
whose lanes start inside the scene in unrelated directions, and directions whose length is far from 1.  This module is
free of torch: tests/test_ray_families_host.py pins the families and references on the CPU, and
tests/test_gpu_ray_families.py compares the kernels with them.

Scenes ("wide", "rtiow", "rects", "mixed"): see scene().  Each has a populated box, BOXES[name]: the region its small
primitives fill.  On "wide" and "rtiow" the 1000-unit ground sphere's own bounds are left out of it: a ray that starts
1000 units from a 0.1-unit sphere has no decidable answer in float32 (b * b - a * c cancels), and the origins are meant
to be ones a caller would send.

Families, each (n, 2, 4) float32 with n <= 960 and fixed seeds ([o, tmin], [d, tmax]; the closest-hit entry points ignore
the two range words, which are 0 there):
  axis      for each signed axis a 16 x 10 grid of origins on a plane outside the populated box on that side, direction
            +-1 along the axis; the two zero components are +0 on even indices and -0 on odd ones (or the other way round).
            The grid is offset by non-round amounts so that no origin coordinate equals a rectangle's plane coordinate.
  planar    origins inside the box; directions with exactly one zero component (+0 or -0), not normalised.
  tiny      the axis rays with one of the two zeros replaced by +-2^-130, a subnormal.
  interior  origins uniform inside the box, directions uniform on the sphere.
  ao        the interior rays with tmin = 0.001 and tmax cycling through 0.25, 1, 4 by index.
  axis_occ  the axis rays with the range (0.001, +inf).
scaled(rays, k) multiplies the directions by 2^k and, with ranges=True, both range ends by 2^-k: all exact.

Decidable: the reference gives the same primitive (or the same occluded) for the ray and for its origin shifted by
+-2^-12 along each axis that moves the ray's line: the two axes perpendicular to an axis or tiny ray, all three
otherwise.  ao also asks for the same answer with tmax * (1 +- 2^-8).  At most UNDECIDABLE_CAP of a case's rays may be
undecidable.  No ray may make the reference compute a NaN t (a ray lying in a rectangle's plane: include/rt_hip.h
leaves its result unspecified); every case asserts that when it is built."""
from __future__ import annotations

import ctypes as C
import functools

import numpy as np

from cudaraytracer_amd import abi, scenes
from cudaraytracer_amd._lib import lib

from test_denoise_host import closest_hits, mixed_scene
from test_occlusion_host import occlusion_reference
from test_query_host import query_scene, records_reference

F = np.float32
SCENES = ("wide", "rtiow", "rects", "mixed")
QUERY_FAMILIES = ("axis", "planar", "tiny", "interior")
OCCLUSION_FAMILIES = ("ao", "axis_occ")
SHIFT = 2.0 ** -12
AO_TMAX = (0.25, 1.0, 4.0)
AXES = ((0, 1.0), (0, -1.0), (1, 1.0), (1, -1.0), (2, 1.0), (2, -1.0))  # (axis, sign): index // 160 of an axis ray
GRID = (16, 10)
TINY = 2.0 ** -130


def small_rects_scene():
    """48 small axis-aligned rectangles (0.3-0.8 units) scattered around the origin, Lambertian."""
    rng = np.random.default_rng(11)
    n = 48
    h = (abi.HittableDesc * n)()
    m = (abi.MaterialDesc * n)()
    for i in range(n):
        h[i].type = (abi.RT_XYRECT, abi.RT_XZRECT, abi.RT_YZRECT)[i % 3]
        h[i].is_active = 1
        h[i].center[:] = [float(v) for v in rng.uniform(-6.0, 6.0, 3).astype(np.float32)]
        h[i].width, h[i].height = (float(v) for v in rng.uniform(0.3, 0.8, 2).astype(np.float32))
        h[i].material = i
        m[i].type = abi.RT_LAMBERTIAN
        m[i].albedo.type = abi.RT_CONSTANT
        m[i].albedo.image = -1
        m[i].albedo.color[:] = [float(v) for v in rng.uniform(0.2, 0.9, 3).astype(np.float32)]
    return scenes.Scene(h, m, [])


@functools.lru_cache(maxsize=None)
def scene(name: str) -> scenes.Scene:
    """"wide": sphere_field(9000, 6), 32-bit BVH references; "rtiow": the built-in, 16-bit references; "rects": the 48
    small rectangles; "mixed": every rectangle type, a checker, an image texture, every material and spheres."""
    if name in ("wide", "rtiow"):
        return query_scene(name)
    return {"rects": small_rects_scene, "mixed": mixed_scene}[name]()


# The populated boxes (lo, hi), and how far outside them the axis rays' planes lie.  "mixed" is a room open towards +x,
# +y and +z: the box stays inside its floor (y = -1), back wall (z = -3), side wall (x = -3.5) and light panel (y = 2.6),
# and reaches 0.9 past the floor's and the walls' edges at x = 4.5 and z = 4.5, where axis rays miss.
BOXES = {"wide": ((-10.0, 0.3, -10.0), (10.0, 2.4, 10.0)),
         "rtiow": ((-10.0, 0.05, -10.0), (10.0, 1.0, 10.0)),
         "rects": ((-6.5, -6.5, -6.5), (6.5, 6.5, 6.5)),
         "mixed": ((-3.4, -0.9, -2.9), (5.4, 2.5, 5.4))}
PLANE_GAP = {"wide": (1.5, 0.8, 1.5), "rtiow": (1.5, 1.3, 1.5), "rects": (1.0, 1.0, 1.0), "mixed": (2.1, 1.6, 2.6)}
SEEDS = {"wide": 101, "rtiow": 102, "rects": 103, "mixed": 104}


def prim_source(sc: scenes.Scene) -> np.ndarray:
    """Per primitive in BVH order the hittable's index in the description (rt_build_host_tables)."""
    desc = sc.desc()
    info = abi.HostTablesInfo()
    assert lib().rt_build_host_tables(C.byref(desc), None, None, None, None, C.byref(info)) == 0
    nodes = (C.c_float * (16 * max(1, info.num_nodes)))()
    prims = (C.c_float * (8 * max(1, info.num_prims)))()
    mats = (C.c_float * (12 * max(1, info.num_materials)))()
    src = (C.c_int32 * max(1, info.num_prims))()
    assert lib().rt_build_host_tables(C.byref(desc), nodes, prims, mats, src, C.byref(info)) == 0
    return np.array(src[: info.num_prims], dtype=np.int32)


# ---------------------------------------------------------------------------------------------------------------------
# The families
# ---------------------------------------------------------------------------------------------------------------------
def _pack(o, d, tmin=0.0, tmax=0.0) -> np.ndarray:
    rays = np.zeros((o.shape[0], 2, 4), dtype=F)
    rays[:, 0, :3], rays[:, 1, :3] = o, d
    rays[:, 0, 3], rays[:, 1, 3] = tmin, tmax
    return rays


def axis(name: str, neg_zero: str = "odd") -> np.ndarray:
    """The axis rays; neg_zero: whether the odd or the even indices carry -0 in their two zero components."""
    lo, hi = (np.array(v) for v in BOXES[name])
    gap = PLANE_GAP[name]
    nu, nv = GRID
    o = np.zeros((6 * nu * nv, 3), dtype=F)
    d = np.zeros((6 * nu * nv, 3), dtype=F)
    for k, (ax, sign) in enumerate(AXES):
        ua, va = (ax + 1) % 3, (ax + 2) % 3
        # cell centres, moved by non-round amounts (no float32 here is a coordinate a scene's rectangle lies at)
        u = lo[ua] + (np.arange(nu) + 0.5) * (hi[ua] - lo[ua]) / nu + 0.00137
        v = lo[va] + (np.arange(nv) + 0.5) * (hi[va] - lo[va]) / nv - 0.00291
        uu, vv = np.meshgrid(u, v, indexing="ij")
        s = slice(k * nu * nv, (k + 1) * nu * nv)
        o[s, ua], o[s, va] = uu.ravel(), vv.ravel()
        o[s, ax] = (lo[ax] - gap[ax] - 0.00173) if sign > 0 else (hi[ax] + gap[ax] + 0.00173)
        d[s, ax] = sign
    idx = np.arange(o.shape[0])
    neg = (idx % 2 == 1) if neg_zero == "odd" else (idx % 2 == 0)
    zero = d == 0
    d[zero & neg[:, None]] = F(-0.0)
    return _pack(o, d)


def tiny(name: str) -> np.ndarray:
    """The axis rays with one zero component (the first on indices 0, 1 mod 4, the second on 2, 3 mod 4) replaced by
    2^-130 of the zero's own sign."""
    rays = axis(name).copy()
    d = rays[:, 1, :3]
    for r in range(d.shape[0]):
        ax = AXES[r // (GRID[0] * GRID[1])][0]
        z = ((ax + 1) % 3, (ax + 2) % 3)[(r // 2) % 2]
        d[r, z] = np.copysign(F(TINY), d[r, z])
    assert np.all((d != 0).sum(1) == 2) and np.all(np.abs(d).min(1) <= F(TINY))
    return rays


def _interior_origins(name: str, rng, n: int) -> np.ndarray:
    """Uniform in the populated box; on "rects" uniform within 0.35 of a rectangle's centre along every axis (uniform in
    the 13-unit box, 2.6 % of the rays would hit one of the 48 small rectangles: too few to show both outcomes)."""
    if name == "rects":
        c = np.array([h.center[:] for h in scene(name).hittables], dtype=np.float64)
        return (c[rng.integers(0, len(c), n)] + rng.uniform(-0.35, 0.35, (n, 3))).astype(F)
    lo, hi = BOXES[name]
    return rng.uniform(lo, hi, (n, 3)).astype(F)


def interior(name: str, n: int = 960) -> np.ndarray:
    rng = np.random.default_rng(SEEDS[name])
    o = _interior_origins(name, rng, n)
    d = rng.standard_normal((n, 3))
    d = (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(F)
    assert np.all(d != 0)
    return _pack(o, d)


def planar(name: str, n: int = 960) -> np.ndarray:
    """96 directions: the zero on each axis as +0 and as -0, the other two components (1, 1), (1, 0.5), (1, 2) and
    (0.25, 3) under all four sign pairs; ray i takes direction i mod 96 from an origin of its own."""
    dirs = []
    for z in range(3):
        for zero in (0.0, -0.0):
            for a, b in ((1.0, 1.0), (1.0, 0.5), (1.0, 2.0), (0.25, 3.0)):
                for sa, sb in ((1, 1), (-1, 1), (1, -1), (-1, -1)):
                    v = [0.0, 0.0, 0.0]
                    v[z], v[(z + 1) % 3], v[(z + 2) % 3] = zero, sa * a, sb * b
                    dirs.append(v)
    dirs = np.array(dirs, dtype=F)
    rng = np.random.default_rng(SEEDS[name] + 1000)
    o = _interior_origins(name, rng, n)
    d = dirs[np.arange(n) % len(dirs)]
    assert np.all((d == 0).sum(1) == 1)
    return _pack(o, d)


def ao(name: str) -> np.ndarray:
    rays = interior(name).copy()
    rays[:, 0, 3] = 0.001
    rays[:, 1, 3] = np.array(AO_TMAX, dtype=F)[np.arange(rays.shape[0]) % 3]
    return rays


def axis_occ(name: str, neg_zero: str = "odd") -> np.ndarray:
    rays = axis(name, neg_zero).copy()
    rays[:, 0, 3], rays[:, 1, 3] = 0.001, np.inf
    return rays


FAMILIES = {"axis": axis, "planar": planar, "tiny": tiny, "interior": interior, "ao": ao, "axis_occ": axis_occ}


def scaled(rays: np.ndarray, k: int, ranges: bool = False) -> np.ndarray:
    """The rays with d * 2^k and, with ranges, tmin * 2^-k and tmax * 2^-k: every product exact (a tmax that overflows
    becomes +inf, which bounds the same rays as FLT_MAX does)."""
    out = np.array(rays, dtype=F)
    out[:, 1, :3] = np.ldexp(out[:, 1, :3], k)
    if ranges:
        with np.errstate(over="ignore"):
            out[:, 0, 3], out[:, 1, 3] = np.ldexp(out[:, 0, 3], -k), np.ldexp(out[:, 1, 3], -k)
    return out


# ---------------------------------------------------------------------------------------------------------------------
# The references
# ---------------------------------------------------------------------------------------------------------------------
def shift_axes(family: str, rays: np.ndarray) -> list:
    """Per ray the axes its origin is shifted along."""
    if family in ("axis", "tiny", "axis_occ"):
        main = np.abs(rays[:, 1, :3]).argmax(1)
        return [((main + 1) % 3), ((main + 2) % 3)]
    n = rays.shape[0]
    return [np.full(n, a) for a in range(3)]


def shifted_origins(family: str, rays: np.ndarray) -> list:
    out = []
    rows = np.arange(rays.shape[0])
    for axes in shift_axes(family, rays):
        for s in (SHIFT, -SHIFT):
            o = rays[:, 0, :3].copy()
            o[rows, axes] += F(s)
            out.append(o)
    return out


def in_plane(sc: scenes.Scene, rays: np.ndarray) -> np.ndarray:
    """(n,) bool: the ray lies in the plane of an active rectangle as the reference computes it: (k - o_k) * (1 / d_k)
    is 0 * inf, a NaN t."""
    o, d = rays[:, 0, :3], rays[:, 1, :3]
    with np.errstate(divide="ignore", over="ignore"):
        inf = np.isinf(F(1.0) / d)
    out = np.zeros(rays.shape[0], dtype=bool)
    for h in sc.hittables:
        if h.is_active and h.type != abi.RT_SPHERE:
            k = {abi.RT_XYRECT: 2, abi.RT_XZRECT: 1, abi.RT_YZRECT: 0}[h.type]
            out |= inf[:, k] & (o[:, k] == F(h.center[k]))
    return out


def _freeze(out: dict) -> dict:
    for a in out.values():
        a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def family_case(name: str, family: str) -> dict:
    """One (scene, family)'s rays and reference, computed once per process and shared (read-only).  A query family: the
    dict of records_reference; an occlusion family: rays, occluded and decidable."""
    sc = scene(name)
    rays = FAMILIES[family](name)
    assert rays.shape[0] <= 960 and rays.dtype == F
    assert not in_plane(sc, rays).any(), (name, family)
    o, d = np.ascontiguousarray(rays[:, 0, :3]), np.ascontiguousarray(rays[:, 1, :3])
    if family in QUERY_FAMILIES:
        ref = records_reference(sc, o, d, [(o2, d) for o2 in shifted_origins(family, rays)])
        assert not np.isnan(ref["normal_depth"]).any(), (name, family)
        return ref
    occluded = occlusion_reference(sc, rays)
    decidable = np.ones(rays.shape[0], dtype=bool)
    variants = []
    for o2 in shifted_origins(family, rays):
        r2 = rays.copy()
        r2[:, 0, :3] = o2
        variants.append(r2)
    if family == "ao":
        for f in (1.0 + 2.0 ** -8, 1.0 - 2.0 ** -8):
            r2 = rays.copy()
            r2[:, 1, 3] *= F(f)
            variants.append(r2)
    for r2 in variants:
        decidable &= (occlusion_reference(sc, r2) == occluded) & ~in_plane(sc, r2)
    return _freeze({"rays": rays, "occluded": occluded, "decidable": decidable})
