"""RT_RADIANCE_DIRECT_LIGHT and rt_scene_lights_host without a device: the constant and the export against the header,
rt_radiance_rays' argument check with the flag, the light list of the built-in and of hand-made scenes, and the density
the estimator rests on.

The density: the reference's Lambertian scatters along normal + RandomInUnitSphere(), a point of the unit ball found by
rejection.  Seen from the hit point, which lies on the surface of the ball about the normal's tip, the ball's chord
along a direction at angle theta from the normal has length 2 mu, mu = cos theta, so the direction's density is
p(omega) = int_0^{2 mu} t^2 dt / (4 pi / 3) = 2 mu^3 / pi.  test_density_of_the_reference_scatter checks it by brute force
against a quadrature of the lamp's solid angle, on the set-up tests/test_gpu_direct_light.py measures on the GPU."""
from __future__ import annotations

import ctypes as C
import functools
import os

import numpy as np

from cudaraytracer_amd import abi, scenes
from cudaraytracer_amd._lib import EXPORTED, lib

from test_radiance_host import _bogus_scene, _radiance_args, _rejected

F = np.float32
HEADER = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "rt_hip.h")).read()
DIRECT = abi.RT_RADIANCE_DIRECT_LIGHT


# ---------------------------------------------------------------------------------------------------------------------
# Hand-made scenes (shared with tests/test_gpu_direct_light.py)
# ---------------------------------------------------------------------------------------------------------------------
def material(kind: int, color=(0.0, 0.0, 0.0), intensity: int = 0, fuzz: float = 0.0) -> abi.MaterialDesc:
    m = abi.MaterialDesc()
    m.type, m.fuzz, m.ir, m.light_intensity = kind, fuzz, 1.5, intensity
    m.albedo.type, m.albedo.image = abi.RT_CONSTANT, -1
    m.albedo.color[:] = color
    return m


def rect(kind: int, center, width: float, height: float, mat: int, active: int = 1) -> abi.HittableDesc:
    h = abi.HittableDesc()
    h.type, h.is_active, h.width, h.height, h.material = kind, active, width, height, mat
    h.center[:] = center
    return h


def sphere(center, radius: float, mat: int, active: int = 1) -> abi.HittableDesc:
    h = abi.HittableDesc()
    h.type, h.is_active, h.radius, h.material = abi.RT_SPHERE, active, radius, mat
    h.center[:] = center
    return h


def make_scene(hittables, materials) -> scenes.Scene:
    return scenes.Scene((abi.HittableDesc * len(hittables))(*hittables), (abi.MaterialDesc * len(materials))(*materials), [])


def lights_of(scene: scenes.Scene, capacity: int | None = None) -> tuple:
    """(count, the entries written) of a direct rt_scene_lights_host call with room for `capacity` entries (None: the
    count of a first call), behind which a guard word must stay."""
    desc = scene.desc()
    count = C.c_uint32(0xdeadbeef)
    assert lib().rt_scene_lights_host(C.byref(desc), None, 0, C.byref(count)) == 0, lib().rt_last_error()
    cap = count.value if capacity is None else capacity
    out = (C.c_uint32 * (cap + 1))(*([0xa5a5a5a5] * (cap + 1)))
    second = C.c_uint32(0)
    assert lib().rt_scene_lights_host(C.byref(desc), out, cap, C.byref(second)) == 0, lib().rt_last_error()
    assert second.value == count.value and out[cap] == 0xa5a5a5a5
    return count.value, list(out[:cap])


@functools.lru_cache(maxsize=None)
def config_scene(name: str) -> scenes.Scene:
    cfg = scenes.CONFIGS[name]
    return scenes.builtin(cfg.scene, texture_size=(64, 32))


def mixed_scene() -> scenes.Scene:
    """A light sphere, an inactive light rectangle, a zero-width and a zero-height one, an intensity-0 one, a Lambertian
    rectangle, and three valid lights of the three types out of order among them."""
    mats = [material(abi.RT_LAMBERTIAN, (0.5, 0.5, 0.5)), material(abi.RT_DIFFUSELIGHT, (1, 1, 1), 4),
            material(abi.RT_DIFFUSELIGHT, (1, 1, 1), 0), material(abi.RT_DIFFUSELIGHT, (1, 0.5, 0.25), 2)]
    hs = [sphere((0, 3, 0), 0.5, 1),                                  # 0: a light, but a sphere
          rect(abi.RT_XZRECT, (0, 0, 0), 10, 10, 0),                  # 1: Lambertian
          rect(abi.RT_YZRECT, (2, 1, 0), 0.5, 0.5, 3),                # 2: valid
          rect(abi.RT_XZRECT, (0, 2, 0), 1, 1, 1, active=0),          # 3: inactive
          rect(abi.RT_XZRECT, (1, 2, 0), 0.0, 1, 1),                  # 4: zero width
          rect(abi.RT_XYRECT, (0, 1, -2), 0.5, 0.25, 1),              # 5: valid
          rect(abi.RT_XZRECT, (-1, 2, 0), 1, 1, 2),                   # 6: intensity 0
          rect(abi.RT_XYRECT, (1, 1, -2), 1, 0.0, 1),                 # 7: zero height
          rect(abi.RT_XZRECT, (0.5, 2, 0.5), 0.6, 0.4, 1)]            # 8: valid
    hs += [sphere((0.3 * k - 3, 0.2, 1.0), 0.1, 0) for k in range(20)]  # (enough primitives for several leaves)
    return make_scene(hs, mats)


# ---------------------------------------------------------------------------------------------------------------------
# The C ABI
# ---------------------------------------------------------------------------------------------------------------------
def test_constant_export_and_header():
    assert DIRECT == 256 and "#define RT_RADIANCE_DIRECT_LIGHT (1u << 8)" in HEADER
    assert "rt_scene_lights_host" in EXPORTED and hasattr(lib(), "rt_scene_lights_host")
    assert "int rt_scene_lights_host(const rt_scene_desc* desc, uint32_t* hittables, uint32_t capacity, uint32_t* count);" in HEADER
    assert lib().rt_abi_version() == 14 and abi.ABI_VERSION == 14 and "#define RT_ABI_VERSION 14" in HEADER
    comment = HEADER[:HEADER.index("#define RT_ABI_VERSION")]
    comment = comment[comment.rindex("/*"):]
    assert "RT_RADIANCE_DIRECT_LIGHT" in comment and "rt_scene_lights_host" in comment
    assert C.sizeof(abi.RadianceArgs) == 120  # (no layout changed)


def test_flag_is_accepted_by_the_argument_check():
    """flags = 256, alone and with the fill order, passes every check (a NULL scene is what stops the call)."""
    L, who = lib(), "rt_radiance_rays"
    for flags in (DIRECT, DIRECT | abi.RT_FLAG_RIUS_LEFT_TO_RIGHT):
        for depth in (0, 1, 8, 4096):
            a, keep = _radiance_args()
            a.flags, a.max_depth = flags, depth
            _rejected(L.rt_radiance_rays(None, C.byref(a), None), who, "NULL scene")
    # without the flag the depth is not limited
    a, keep = _radiance_args()
    a.max_depth = 4097
    _rejected(L.rt_radiance_rays(None, C.byref(a), None), who, "NULL scene")


def test_flag_rejections():
    L, scene, who = lib(), _bogus_scene(), "rt_radiance_rays"
    for depth in (4097, 1 << 16, 0xffffffff):
        a, keep = _radiance_args()
        a.flags, a.max_depth = DIRECT, depth
        _rejected(L.rt_radiance_rays(scene, C.byref(a), None), who, "max_depth")
    # every flag bit tests/test_radiance_host.py lists as bad, with the new flag beside it
    for bad in (1, 2, 4, 16, abi.RT_FLAG_RNG_PHILOX, 64, 128, 1 << 31, abi.RT_FLAG_RIUS_LEFT_TO_RIGHT | 1, 512, 1 << 9 | 8):
        for with_flag in (0, DIRECT):
            a, keep = _radiance_args()
            a.flags = bad | with_flag
            _rejected(L.rt_radiance_rays(scene, C.byref(a), None), who, "flags")
    for k in range(3):
        for bad in (1, 1 << 31):
            a, keep = _radiance_args()
            a.flags, a.reserved[k] = DIRECT, bad
            _rejected(L.rt_radiance_rays(scene, C.byref(a), None), who, "reserved")


def test_no_rays_with_the_flag_needs_no_device():
    a, keep = _radiance_args(0)
    a.flags = DIRECT
    assert lib().rt_radiance_rays(None, C.byref(a), None) == 0
    a.max_depth = 4097  # ... but the arguments are still checked
    _rejected(lib().rt_radiance_rays(None, C.byref(a), None), "rt_radiance_rays", "max_depth")


# ---------------------------------------------------------------------------------------------------------------------
# rt_scene_lights_host
# ---------------------------------------------------------------------------------------------------------------------
def test_lights_of_the_builtin_scenes():
    assert lights_of(config_scene("c3")) == (1, [2])
    assert scenes.scene_lights(config_scene("c3")) == [2]
    h = config_scene("c3").hittables[2]
    m = config_scene("c3").materials[h.material]
    assert h.type == abi.RT_XZRECT and (h.width, h.height) == (130.0, 105.0) and m.type == abi.RT_DIFFUSELIGHT
    for name in ("c1", "c2", "c5"):
        assert lights_of(config_scene(name)) == (0, []), name
        assert scenes.scene_lights(config_scene(name)) == []
    # c5's "sun" is an emitter, but a sphere: not sampled
    c5 = config_scene("c5")
    assert any(c5.materials[h.material].type == abi.RT_DIFFUSELIGHT and h.type == abi.RT_SPHERE for h in c5.hittables)


def test_lights_of_a_mixed_list():
    s = mixed_scene()
    assert lights_of(s) == (3, [2, 5, 8])
    assert scenes.scene_lights(s) == [2, 5, 8]
    # the order and the list do not depend on the BVH: leaf sizes 1..4 build different trees over the same list
    info = abi.HostTablesInfo()
    nodes = set()
    for leaf_max in (1, 2, 3, 4):
        prev = lib().rt_set_tuning(abi.RT_TUNE_LEAF_MAX, leaf_max)
        try:
            assert lights_of(s) == (3, [2, 5, 8]), leaf_max
            desc = s.desc()
            assert lib().rt_build_host_tables(C.byref(desc), None, None, None, None, C.byref(info)) == 0
            nodes.add(info.num_nodes)
        finally:
            lib().rt_set_tuning(abi.RT_TUNE_LEAF_MAX, prev)
    assert len(nodes) > 1  # (the trees did differ)
    # a material edit's effect on the list: rectangle 6 becomes a light, 5 and 8 stop being one
    s.materials[2].light_intensity = 1
    s.materials[1].type = abi.RT_LAMBERTIAN
    assert lights_of(s) == (2, [2, 6])


def test_capacity_bounds_what_is_written():
    s = mixed_scene()
    assert lights_of(s, 0) == (3, [])
    assert lights_of(s, 1) == (3, [2])
    assert lights_of(s, 2) == (3, [2, 5])
    assert lights_of(s, 5) == (3, [2, 5, 8, 0xa5a5a5a5, 0xa5a5a5a5])


def test_lights_host_errors_are_scene_creation_errors():
    L = lib()
    count = C.c_uint32(7)
    assert L.rt_scene_lights_host(None, None, 0, C.byref(count)) == -1 and b"rt_scene_lights_host" in L.rt_last_error()
    s = mixed_scene()
    desc = s.desc()
    assert L.rt_scene_lights_host(C.byref(desc), None, 0, None) == -1
    assert L.rt_scene_lights_host(C.byref(desc), None, 4, C.byref(count)) == -1  # NULL with a capacity
    s.hittables[2].material = 99
    desc = s.desc()
    assert L.rt_scene_lights_host(C.byref(desc), None, 0, C.byref(count)) == -2 and b"material index" in L.rt_last_error()
    s = mixed_scene()
    s.hittables[5].width = float("nan")
    desc = s.desc()
    assert L.rt_scene_lights_host(C.byref(desc), None, 0, C.byref(count)) == -2 and b"non-finite" in L.rt_last_error()
    s = mixed_scene()
    s.materials[1].type = 9
    desc = s.desc()
    assert L.rt_scene_lights_host(C.byref(desc), None, 0, C.byref(count)) == -2
    empty = make_scene([], [material(abi.RT_LAMBERTIAN)])
    assert lights_of(empty) == (0, [])


# ---------------------------------------------------------------------------------------------------------------------
# The density
# ---------------------------------------------------------------------------------------------------------------------
LAMP_CENTER, LAMP_SIZE = (0.5, 1.0, 0.0), (0.6, 0.4)  # an XZ lamp one unit above the floor y = 0
FLOOR_POINT = (0.3, 0.0, 0.2)


def lamp_quadrature(p, center=LAMP_CENTER, size=LAMP_SIZE, n: int = 1024) -> float:
    """int over the lamp of 2 cos^3(theta) / pi * cos(theta') / d^2 dA for the floor point p (normal +y), float64
    midpoint rule on n x n cells: the probability that the reference's Lambertian direction at p meets the lamp."""
    xs = center[0] + ((np.arange(n) + 0.5) / n - 0.5) * size[0]
    zs = center[2] + ((np.arange(n) + 0.5) / n - 0.5) * size[1]
    vx, vz = xs[:, None] - p[0], zs[None, :] - p[2]
    vy = center[1] - p[1]
    d2 = vx * vx + vy * vy + vz * vz
    c = vy / np.sqrt(d2)  # cos theta = cos theta' (parallel planes)
    return float((2.0 * c ** 3 / np.pi * c / d2).sum() * (size[0] / n) * (size[1] / n))


def test_density_of_the_reference_scatter():
    """Brute force — normal + a uniform point of the unit ball, by rejection as RandomInUnitSphere finds it — against the
    quadrature of 2 cos^3 / pi over the lamp, within 5 standard errors of the brute-force run."""
    rng = np.random.default_rng(1984)
    total, hits = 0, 0
    for _ in range(4):
        q = rng.uniform(-1.0, 1.0, (3_000_000, 3))
        q = q[(q * q).sum(axis=1) < 1.0]
        d = q + np.array([0.0, 1.0, 0.0])
        up = d[:, 1] > 0
        t = (LAMP_CENTER[1] - FLOOR_POINT[1]) / d[up, 1]
        x, z = FLOOR_POINT[0] + t * d[up, 0], FLOOR_POINT[2] + t * d[up, 2]
        hits += int(((np.abs(x - LAMP_CENTER[0]) <= LAMP_SIZE[0] / 2) & (np.abs(z - LAMP_CENTER[2]) <= LAMP_SIZE[1] / 2)).sum())
        total += q.shape[0]
    p = hits / total
    se = (p * (1 - p) / total) ** 0.5
    quad = lamp_quadrature(FLOOR_POINT)
    print(f"brute force {p:.5f} +- {se:.5f} ({total} samples), quadrature {quad:.5f}")
    assert total > 6_000_000 and 0.10 < quad < 0.12
    assert abs(p - quad) <= 5 * se
    # the quadrature has converged: half the cells give the same figure to 1e-7
    assert abs(lamp_quadrature(FLOOR_POINT, n=512) - quad) < 1e-7
