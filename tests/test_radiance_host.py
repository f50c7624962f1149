"""rt_radiance_rays and rt_camera_rays without a device: the structs against the header, the exports, every argument
check, and the reference that tests/test_gpu_radiance.py compares the kernels with.

The reference is the oracle alone.  In Philox mode a frame's samples do not depend on one another, and a pixel's sum
is kept in 2^-12 fixed point, so sample s of every pixel is the difference of two oracle frames:

    sample_reference(frame, s) = 4096 * (accum after spp = s + 1  -  accum after spp = s)      (uint32 per channel)

with the geometric closest hit (OracleScene(exact=True)), which is rt_radiance_rays' definition.  The tests here assert
that the differences are whole numbers of 2^-12 units, and that on the frames of the GPU test the oracle with the
reference BVH's culling (exact=False) gives the same samples on every pixel — no ray of these frames sits on a tie or
a culling edge — so the GPU comparison may demand every ray, bit for bit."""
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

from test_query_host import query_cameras, query_scene

F = np.float32
HEADER = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "rt_hip.h")).read()
SAMPLES = 3  # samples 0..2 of every frame
SLOT = 8192  # bytes between the dummy buffers of the argument tests (the largest holds 128 rays: 4096)
SEED = 1984


# ---------------------------------------------------------------------------------------------------------------------
# The frames and their reference
# ---------------------------------------------------------------------------------------------------------------------
def _config_frame(name, size, depth=None, texture_size=None):
    cfg = scenes.CONFIGS[name]
    return (lambda: scenes.builtin(cfg.scene, texture_size=texture_size or cfg.texture_size), cfg.inputs, size,
            depth if depth is not None else cfg.depth)


# name: (scene, inputs, (width, height), depth): the smallest frames with partial waves, several waves and every material
FRAMES = {
    "c1": _config_frame("c1", (48, 32)),
    "default": _config_frame("default", (48, 32), depth=8),
    "c2_40x24": _config_frame("c2", (40, 24)),
    "c2_37x21": _config_frame("c2", (37, 21)),
    "c3": _config_frame("c3", (32, 32), depth=8),  # rectangles, emitters, a black sky
    "c5": _config_frame("c5", (48, 32), texture_size=(64, 32)),
    "wide_near": (lambda: query_scene("wide"), lambda: query_cameras()["near"], (37, 21), 6),  # 32-bit references
    "wide_far": (lambda: query_scene("wide"), lambda: query_cameras()["far"], (37, 21), 6),
}


@functools.lru_cache(maxsize=None)
def frame_scene(name: str) -> scenes.Scene:
    return FRAMES[name][0]()


def frame_inputs(name: str) -> abi.InputStruct:
    return FRAMES[name][1]()


@functools.lru_cache(maxsize=None)
def _oracle_sums(name: str, exact: bool, rius_order: int) -> tuple:
    """accum (W·H, 3) float64 and the ray count after spp = 0 .. SAMPLES of the frame's Philox render."""
    _, _, (w, h), depth = FRAMES[name]
    osc = po.OracleScene(frame_scene(name), exact=exact)
    sums, rays = [np.zeros((w * h, 3))], [0]
    for spp in range(1, SAMPLES + 1):
        acc = np.zeros(w * h * 4, dtype=F)
        _, _, cnt = po.render(osc, w, h, spp, depth, frame_inputs(name), None, philox=True, seed=SEED, frame=0,
                              accum=acc, rius_order=rius_order, threads=8)
        acc = acc.reshape(w * h, 4)
        assert np.all(acc[:, 3] == spp)
        sums.append(acc[:, :3].astype(np.float64))
        rays.append(int(cnt.rays))
    return sums, rays


def sample_reference(name: str, s: int, exact: bool = True, rius_order: int = 1) -> tuple:
    """Sample s of every pixel of the frame, (W·H, 3) uint32 in 2^-12 units indexed by the global pixel index, and the
    rays (color() iterations) the sample took over the frame."""
    sums, rays = _oracle_sums(name, exact, rius_order)
    d = 4096.0 * (sums[s + 1] - sums[s])
    assert np.all(d >= 0) and np.all(d == np.round(d)) and d.max() < 2.0 ** 24, name  # whole units, exact in float
    q = d.astype(np.uint32)
    q.setflags(write=False)
    return q, rays[s + 1] - rays[s]


@pytest.mark.parametrize("name", list(FRAMES))
def test_reference_samples(name):
    """Whole 2^-12 units; the exact and the reference-BVH oracle agree on every pixel and sample; the frame is not
    trivial (lit and varied)."""
    differing, total = 0, 0
    for s in range(SAMPLES):
        q, rays = sample_reference(name, s)
        q2, rays2 = sample_reference(name, s, exact=False)
        differing += int(np.any(q != q2, axis=1).sum())
        total += q.shape[0]
        assert rays == rays2
        w, h = FRAMES[name][2]
        assert w * h <= rays <= w * h * FRAMES[name][3]
        # (not a blank frame: the box of c3 is the darkest, a path there ends at the small light or at the depth limit)
        assert len(np.unique(q, axis=0)) > 8 and np.any(q != 0, axis=1).mean() > 0.01
    print(f"{name}: differing share {differing / total:.4f}")
    assert differing == 0


def test_reference_fill_order_matters():
    """The two Random() fill orders give different samples on the frame the GPU test runs both on."""
    a, _ = sample_reference("c2_37x21", 0)
    b, _ = sample_reference("c2_37x21", 0, rius_order=0)
    assert np.any(a != b)


# ---------------------------------------------------------------------------------------------------------------------
# The C ABI
# ---------------------------------------------------------------------------------------------------------------------
def _header_fields(struct: str) -> list:
    """[(type text, name, array length or 0)] of a struct of the header, in order."""
    m = re.search(r"typedef struct %s \{(.*?)\} %s;" % (struct, struct), HEADER, re.S)
    assert m, struct
    body = re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S)
    out = []
    for decl in (d.strip() for d in body.split(";")):
        if not decl:
            continue
        type_text, names = decl.rsplit(None, 1) if "," not in decl else decl.split(None, 1)
        for nm in names.split(","):
            nm = nm.strip()
            arr = re.search(r"\[(\d+)\]", nm)
            out.append((type_text + ("*" if "*" in nm else ""), re.sub(r"[\s*]|\[\d+\]", "", nm), int(arr.group(1)) if arr else 0))
    return out


C_SIZES = {"uint32_t": 4, "float": 4, "uint64_t": 8, "rt_tiling": 16, "rt_input_struct": 72}


def _check_layout(struct: str, mirror, size: int) -> None:
    fields = _header_fields(struct)
    assert [f[1] for f in fields] == [f[0] for f in mirror._fields_]
    offset = 0
    for type_text, name, arr in fields:
        width = 8 if "*" in type_text else C_SIZES[type_text.replace("const ", "").strip()]
        align = min(width, 8) if type_text.strip() not in ("rt_tiling", "rt_input_struct") else 4
        offset = (offset + align - 1) // align * align
        assert getattr(mirror, name).offset == offset, (struct, name)
        assert getattr(mirror, name).size == width * max(1, arr), (struct, name)
        offset += width * max(1, arr)
    assert C.sizeof(mirror) == size == (offset + 7) // 8 * 8


def test_structs_match_the_header():
    _check_layout("rt_camera_rays_args", abi.CameraRaysArgs, 160)
    _check_layout("rt_radiance_args", abi.RadianceArgs, 120)
    assert [f[1] for f in _header_fields("rt_radiance_args")][:5] == ["rays", "stream_ids", "sum", "mean", "counters"]
    assert [f[1] for f in _header_fields("rt_camera_rays_args")][:3] == ["rays", "pixels", "pixel_index"]
    assert abi.CameraRaysArgs.reserved.size == 8 and abi.RadianceArgs.reserved.size == 12
    assert "#define RT_CAMERA_JITTER_PHILOX 1u" in HEADER and abi.RT_CAMERA_JITTER_PHILOX == 1


def test_exports_and_abi_version():
    for name in ("rt_camera_rays", "rt_radiance_rays"):
        assert name in EXPORTED
        assert hasattr(lib(), name)
    assert lib().rt_abi_version() == 14 and abi.ABI_VERSION == 14  # (additions that change no layout)
    assert "#define RT_ABI_VERSION 14" in HEADER
    comment = HEADER[:HEADER.index("#define RT_ABI_VERSION")]
    comment = comment[comment.rindex("/*"):]
    assert "rt_camera_rays" in comment and "rt_radiance_rays" in comment


def _rejected(rc: int, who: str, what: str | None = None) -> None:
    assert rc == -1, rc
    msg = lib().rt_last_error()
    assert who.encode() in msg, msg
    if what:
        assert what.encode() in msg, msg


# ----- rt_radiance_rays ----------------------------------------------------------------------------------------------
def _radiance_args(n: int = 64):
    """Valid arguments over host dummies (never dereferenced: every check precedes the first device call)."""
    arena = C.create_string_buffer(5 * SLOT)  # one slot each, so a shifted buffer meets only the one it is aimed at
    a = abi.RadianceArgs()
    for k, name in enumerate(("rays", "stream_ids", "sum", "mean", "counters")):
        setattr(a, name, C.addressof(arena) + k * SLOT)
    bufs = arena
    a.n, a.samples_per_ray, a.max_depth = n, 1, 8
    return a, bufs


def _bogus_scene():
    return C.cast(C.create_string_buffer(64), C.c_void_p)  # never dereferenced: the arguments are checked first


def test_radiance_rejects_bad_arguments():
    L, scene, who = lib(), _bogus_scene(), "rt_radiance_rays"
    call = lambda a, s=scene: L.rt_radiance_rays(s, C.byref(a), None)  # noqa: E731
    _rejected(L.rt_radiance_rays(scene, None, None), who, "NULL args")
    a, keep = _radiance_args()
    _rejected(call(a, None), who, "NULL scene")
    a, keep = _radiance_args()
    a.rays = None
    _rejected(call(a), who, "NULL rays")
    a, keep = _radiance_args()
    a.sum = a.mean = None
    _rejected(call(a), who, "no output")
    for bad in (17, 64, 0xffffffff):
        a, keep = _radiance_args()
        a.rays_per_lane = bad
        _rejected(call(a), who, "rays_per_lane")
    for bad in (2, 3, 1 << 31, 0xffffffff):
        a, keep = _radiance_args()
        a.count_tests = bad
        _rejected(call(a), who, "count_tests")
    a, keep = _radiance_args()
    a.count_tests, a.counters = 1, None
    _rejected(call(a), who, "without counters")
    # every flag of rt_render but the fill order, and unknown bits
    for bad in (1, 2, 4, 16, abi.RT_FLAG_RNG_PHILOX, 64, 128, 1 << 31, abi.RT_FLAG_RIUS_LEFT_TO_RIGHT | 1):
        a, keep = _radiance_args()
        a.flags = bad
        _rejected(call(a), who, "flags")
    for k in range(3):
        for bad in (1, 1 << 31):
            a, keep = _radiance_args()
            a.reserved[k] = bad
            _rejected(call(a), who, "reserved")
    a, keep = _radiance_args()
    a.samples_per_ray = 0
    _rejected(call(a), who, "samples_per_ray")
    for base, k in ((0, abi.PHILOX_MAX_SPP + 1), (abi.PHILOX_MAX_SPP, 1), (1, abi.PHILOX_MAX_SPP), (0xffffffff, 1),
                    (1, 0xffffffff), (0xffffffff, 0xffffffff)):
        a, keep = _radiance_args()
        a.sample_base, a.samples_per_ray = base, k
        _rejected(call(a), who, "RT_PHILOX_MAX_SPP")
    # valid: the limits themselves, each output alone, no ids, depth 0, the fill-order flag (a NULL scene stops the call)
    for base, k in ((0, abi.PHILOX_MAX_SPP), (abi.PHILOX_MAX_SPP - 1, 1)):
        a, keep = _radiance_args()
        a.sample_base, a.samples_per_ray = base, k
        _rejected(call(a, None), who, "NULL scene")
    for only in ("sum", "mean"):
        a, keep = _radiance_args()
        setattr(a, "mean" if only == "sum" else "sum", None)
        a.count_tests, a.rays_per_lane, a.stream_ids, a.max_depth = 1, 16, None, 0
        a.flags = abi.RT_FLAG_RIUS_LEFT_TO_RIGHT
        _rejected(call(a, None), who, "NULL scene")


RADIANCE_OUTPUTS = (("sum", 16 * 64), ("mean", 16 * 64), ("counters", abi.COUNTERS_WORDS * 8))  # name, bytes at n = 64


def test_radiance_rejects_overlapping_buffers():
    """An output, counters included, may share no byte with `rays`, `stream_ids` or another output."""
    L, scene, who = lib(), _bogus_scene(), "rt_radiance_rays"
    for name, _ in RADIANCE_OUTPUTS:
        for inp, nbytes in (("rays", 64 * 32), ("stream_ids", 64 * 4)):
            a, keep = _radiance_args()
            setattr(a, name, getattr(a, inp))
            _rejected(L.rt_radiance_rays(scene, C.byref(a), None), who, "overlaps " + inp)
            a, keep = _radiance_args()
            setattr(a, name, getattr(a, inp) + nbytes - 1)  # the input's last byte
            _rejected(L.rt_radiance_rays(scene, C.byref(a), None), who, "overlaps " + inp)
    for i, (first, nbytes) in enumerate(RADIANCE_OUTPUTS):
        for second, _ in RADIANCE_OUTPUTS[i + 1:]:
            a, keep = _radiance_args()
            setattr(a, second, getattr(a, first))
            _rejected(L.rt_radiance_rays(scene, C.byref(a), None), who, "overlap")
            a, keep = _radiance_args()
            setattr(a, second, getattr(a, first) + nbytes - 1)
            _rejected(L.rt_radiance_rays(scene, C.byref(a), None), who, "overlap")
    a, keep = _radiance_args()
    big = C.create_string_buffer(64 * 32)
    a.sum, a.mean = C.addressof(big), C.addressof(big) + 64 * 16  # adjacent, not overlapping
    _rejected(L.rt_radiance_rays(None, C.byref(a), None), who, "NULL scene")


def test_radiance_no_rays_is_accepted_without_a_device():
    a, keep = _radiance_args(0)
    assert lib().rt_radiance_rays(None, C.byref(a), None) == 0
    a.rays = None
    assert lib().rt_radiance_rays(None, C.byref(a), None) == 0
    # ... but the arguments are still checked
    a.flags = 1
    _rejected(lib().rt_radiance_rays(None, C.byref(a), None), "rt_radiance_rays", "flags")
    a.flags, a.samples_per_ray = 0, 0
    _rejected(lib().rt_radiance_rays(None, C.byref(a), None), "rt_radiance_rays", "samples_per_ray")


# ----- rt_camera_rays ------------------------------------------------------------------------------------------------
def _camera_args(n: int = 64, sparse: bool = False):
    """Valid arguments over host dummies: an 8 x 8 frame in one band, or n listed pixels."""
    arena = C.create_string_buffer(3 * SLOT)
    a = abi.CameraRaysArgs()
    for k, name in enumerate(("rays", "pixel_index", "pixels")[:3 if sparse else 2]):
        setattr(a, name, C.addressof(arena) + k * SLOT)
    bufs = arena
    a.n, a.width, a.height = n, 8, 8
    a.tiling = abi.Tiling(8, 1, 0, n // 8)
    a.inputs = scenes.CONFIGS["c2"].inputs()
    a.xi1 = a.xi2 = 0.5
    return a, bufs


def test_camera_rejects_bad_arguments():
    L, who = lib(), "rt_camera_rays"
    call = lambda a: L.rt_camera_rays(C.byref(a), None)  # noqa: E731
    _rejected(L.rt_camera_rays(None, None), who, "NULL args")
    for sparse in (False, True):
        a, keep = _camera_args(sparse=sparse)
        a.rays = None
        _rejected(call(a), who, "NULL rays")
        for bad in (2, 4, 1 << 31, 3):
            a, keep = _camera_args(sparse=sparse)
            a.flags = bad
            _rejected(call(a), who, "flags")
        for k in (0, 1):
            a, keep = _camera_args(sparse=sparse)
            a.reserved[k] = 7
            _rejected(call(a), who, "reserved")
        for bad in (abi.PHILOX_MAX_SPP, 0xffffffff):
            a, keep = _camera_args(sparse=sparse)
            a.flags, a.sample = abi.RT_CAMERA_JITTER_PHILOX, bad
            _rejected(call(a), who, "sample")
    # dense: n must be the tiling's pixel count, and the tiling must be valid and inside the frame
    for n in (63, 65, 0, 8):
        a, keep = _camera_args()
        a.n = n
        _rejected(call(a), who, "local_rows * width")
    for tiling in ((0, 1, 0, 8), (8, 0, 0, 8), (8, 2, 2, 8)):
        a, keep = _camera_args()
        a.tiling = abi.Tiling(*tiling)
        _rejected(call(a), who, "tiling")
    a, keep = _camera_args()
    a.tiling = abi.Tiling(8, 2, 1, 8)  # rank 1's band of an 8-row frame lies outside it
    _rejected(call(a), who, "outside the image")
    a, keep = _camera_args(128)
    a.tiling = abi.Tiling(8, 1, 0, 16)  # 16 rows of an 8-row frame
    _rejected(call(a), who, "outside the image")


def test_camera_rejects_overlapping_buffers():
    L, who = lib(), "rt_camera_rays"
    a, keep = _camera_args(sparse=True)
    a.rays = a.pixels
    _rejected(L.rt_camera_rays(C.byref(a), None), who, "overlaps pixels")
    a, keep = _camera_args(sparse=True)
    a.pixel_index = a.pixels + 64 * 4 - 1
    _rejected(L.rt_camera_rays(C.byref(a), None), who, "overlaps pixels")
    a, keep = _camera_args(sparse=True)
    a.pixels = a.rays + 64 * 32 - 1
    _rejected(L.rt_camera_rays(C.byref(a), None), who, "overlaps pixels")
    for sparse in (False, True):
        a, keep = _camera_args(sparse=sparse)
        a.pixel_index = a.rays + 64 * 32 - 1
        _rejected(L.rt_camera_rays(C.byref(a), None), who, "overlap each other")
        a, keep = _camera_args(sparse=sparse)
        a.pixel_index = a.rays
        _rejected(L.rt_camera_rays(C.byref(a), None), who, "overlap each other")


def test_camera_no_rays_is_accepted_without_a_device():
    a, keep = _camera_args(0)
    assert lib().rt_camera_rays(C.byref(a), None) == 0
    a, keep = _camera_args(0, sparse=True)
    a.rays = None
    assert lib().rt_camera_rays(C.byref(a), None) == 0
    a.flags = 2  # ... but the arguments are still checked
    _rejected(lib().rt_camera_rays(C.byref(a), None), "rt_camera_rays", "flags")
