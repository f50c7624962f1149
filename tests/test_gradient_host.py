"""rt_temporal_gradient and rt_history_adapt without a device: the structs against the header, the exports, every
argument check, the numpy restatements that tests/test_gpu_gradient.py compares the kernels with, the premise of the
pass and its effect on the history's error, both from oracle frames.

gradient_reference restates the comparison of include/rt_hip.h in float32 on two colour planes (the previous frame's
radiance and the re-traced one); adapt_reference restates rt_history_adapt: multiplications, additions, comparisons and
one IEEE division, one rounding each, so the kernels must equal both bit for bit.  The colours come from the oracle
alone: sample s of the edited scenes is the difference of two oracle Philox frames in 2^-12 units, as
tests/test_radiance_host.py sample_reference is for the unedited ones.

The premise: a Philox frame traced again in an edited scene differs in a subset of the pixels only, bit-identical
elsewhere, and on these edited scenes the geometric closest hit and the reference BVH's agree on every pixel.  The
quality tests restate the pipeline after an edit (32 frames of history, the edit, six more frames, max_history 32)
with the real definitions and compare the history's squared error against 512 spp of the edited scene for plain
continuation, a full reset and the adapted lengths (DESIGN.md §19 holds the figures)."""
from __future__ import annotations

import ctypes as C
import functools

import numpy as np
import pytest

from cudaraytracer_amd import abi, scenes
from cudaraytracer_amd._lib import EXPORTED, lib
from oracle import py_oracle as po

from test_radiance_host import (FRAMES, HEADER, SAMPLES, SEED, _check_layout, _header_fields, _rejected, frame_inputs,
                                frame_scene, sample_reference)

F = np.float32
SLOT = 1 << 16  # bytes between the dummy buffers of the argument tests (the largest, a 16 x 8 float4 plane: 2048)


# ---------------------------------------------------------------------------------------------------------------------
# The edits and the oracle's frames of the edited scenes
# ---------------------------------------------------------------------------------------------------------------------
def move(i: int, dx: float):
    def edit(s: scenes.Scene) -> None:
        s.hittables[i].center[0] += dx
    return edit


def recolor(i: int, rgb: tuple):
    def edit(s: scenes.Scene) -> None:
        m = s.hittables[i].material
        for c in range(3):
            s.materials[m].albedo.color[c] = rgb[c]
    return edit


# frame name: the edit the GPU test re-traces it under (one sphere moved by +0.3 in x; wide_near: a sphere 2.3 in front of
# the camera, which changes 13 % of the frame's pixels)
EDITS = {"c2_40x24": move(487, 0.3), "c2_37x21": move(487, 0.3), "c5": move(2, 0.3), "wide_near": move(4443, 0.3)}


def edited(scene: scenes.Scene, edit) -> scenes.Scene:
    out = scenes.Scene.from_bytes(scene.hittables_bytes(), scene.materials_bytes(), scene.images)
    edit(out)
    return out


@functools.lru_cache(maxsize=None)
def edited_scene(name: str) -> scenes.Scene:
    return edited(frame_scene(name), EDITS[name])


@functools.lru_cache(maxsize=None)
def _edited_sums(name: str, exact: bool, rius_order: int) -> list:
    _, _, (w, h), depth = FRAMES[name]
    osc = po.OracleScene(edited_scene(name), exact=exact)
    sums = [np.zeros((w * h, 3))]
    for spp in range(1, SAMPLES + 1):
        acc = np.zeros(w * h * 4, dtype=F)
        po.render(osc, w, h, spp, depth, frame_inputs(name), None, philox=True, seed=SEED, frame=0, accum=acc,
                  rius_order=rius_order, threads=8)
        sums.append(acc.reshape(w * h, 4)[:, :3].astype(np.float64))
    return sums


def edited_reference(name: str, s: int, exact: bool = True, rius_order: int = 1) -> np.ndarray:
    """Sample s of every pixel of the frame in its edited scene, (W·H, 3) uint32 in 2^-12 units (sample_reference's
    form)."""
    sums = _edited_sums(name, exact, rius_order)
    d = 4096.0 * (sums[s + 1] - sums[s])
    assert np.all(d >= 0) and np.all(d == np.round(d)) and d.max() < 2.0 ** 24, name
    q = d.astype(np.uint32)
    q.setflags(write=False)
    return q


# ---------------------------------------------------------------------------------------------------------------------
# The numpy restatements
# ---------------------------------------------------------------------------------------------------------------------
def mean_color(units: list) -> np.ndarray:
    """The mean of k samples given in 2^-12 units, (n, 3) uint32 each, as rt_radiance_rays' `mean` and a k-spp frame's
    radiance plane compute it: the saturating sum, · 2^-12, / k."""
    total = np.minimum(sum(u.astype(np.uint64) for u in units), np.uint64(0xffffffff))
    return ((total.astype(F) * F(1.0 / 4096.0)).astype(F) / F(len(units))).astype(F)


def strata_pixels(w: int, h: int, stride: int, offset: tuple) -> np.ndarray:
    """The global pixel index of every stratum, (SH·SW,) uint32 in stratum order."""
    sw, sh = -(-w // stride), -(-h // stride)
    xs = np.minimum(np.arange(sw) * stride + offset[0], w - 1)
    ys = np.minimum(np.arange(sh) * stride + offset[1], h - 1)
    return (ys[:, None] * w + xs[None, :]).reshape(-1).astype(np.uint32)


def gradient_reference(c_old: np.ndarray, c_new: np.ndarray, w: int, h: int, stride: int, offset: tuple = (0, 0)) -> dict:
    """rt_temporal_gradient's outputs from the two colour planes, (W·H, 3) float32 indexed by the global pixel index:
    {"gradient": (S, 2), "resample": (S, 4), "pixel": (S,) uint32}."""
    pix = strata_pixels(w, h, stride, offset)
    n, o = np.asarray(c_new, dtype=F)[pix], np.asarray(c_old, dtype=F)[pix]
    with np.errstate(invalid="ignore", over="ignore"):
        a = np.abs((n - o).astype(F))
        delta = ((a[:, 0] + a[:, 1]).astype(F) + a[:, 2]).astype(F)
        m = np.where(n > o, n, o).astype(F)
        level = ((m[:, 0] + m[:, 1]).astype(F) + m[:, 2]).astype(F)
    return {"gradient": np.stack([delta, level], axis=1).astype(F),
            "resample": np.concatenate([n, np.ones((len(pix), 1), dtype=F)], axis=1).astype(F), "pixel": pix}


def adapt_factor(gradient: np.ndarray, sw: int, sh: int, radius: int, power: int, gain: float, lum_floor: float) -> np.ndarray:
    """f of rt_history_adapt_args per stratum, (SH, SW) float32, from the (S, 2) gradient plane."""
    g = np.asarray(gradient, dtype=F).reshape(sh, sw, 2)
    D, M, n = np.zeros((sh, sw), dtype=F), np.zeros((sh, sw), dtype=F), np.zeros((sh, sw), dtype=F)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        for dy in range(-radius, radius + 1):      # every stratum adds its neighbours in this order
            for dx in range(-radius, radius + 1):
                y0, y1, x0, x1 = max(0, -dy), min(sh, sh - dy), max(0, -dx), min(sw, sw - dx)
                if y0 >= y1 or x0 >= x1:
                    continue
                D[y0:y1, x0:x1] = (D[y0:y1, x0:x1] + g[y0 + dy:y1 + dy, x0 + dx:x1 + dx, 0]).astype(F)
                M[y0:y1, x0:x1] = (M[y0:y1, x0:x1] + g[y0 + dy:y1 + dy, x0 + dx:x1 + dx, 1]).astype(F)
                n[y0:y1, x0:x1] += F(1.0)
        lo = (F(lum_floor) * n).astype(F)
        q = ((F(gain) * D).astype(F) / np.where(M > lo, M, lo).astype(F)).astype(F)
        keep = (F(1.0) - np.where(q < F(1.0), q, F(1.0)).astype(F)).astype(F)
        f = keep.copy()
        for _ in range(power - 1):
            f = (f * keep).astype(F)
    return f


def adapt_reference(gradient: np.ndarray, history_w: np.ndarray, w: int, h: int, stride: int, radius: int = 1,
                    power: int = 4, gain: float = 1.0, lum_floor: float = 0.01) -> np.ndarray:
    """history.w after rt_history_adapt, (W·H,) float32, from the (S, 2) gradient plane and the lengths before."""
    sw, sh = -(-w // stride), -(-h // stride)
    f = adapt_factor(gradient, sw, sh, radius, power, gain, lum_floor)
    per_pixel = f[(np.arange(h) // stride)[:, None], (np.arange(w) // stride)[None, :]].reshape(-1)
    with np.errstate(invalid="ignore", over="ignore"):
        return (np.asarray(history_w, dtype=F).reshape(-1) * per_pixel).astype(F)


def synthetic_gradient(sw: int, sh: int, seed: int) -> np.ndarray:
    """A gradient plane with every kind of value: mostly exact zeros, small and large differences, an inf and a NaN."""
    rng = np.random.default_rng(seed)
    n = sw * sh
    level = rng.gamma(2.0, 0.4, n).astype(F)
    delta = np.where(rng.random(n) < 0.6, 0.0, rng.gamma(1.0, 0.2, n)).astype(F)
    delta[rng.integers(0, n, max(1, n // 40))] = F(1e4)
    level[rng.integers(0, n, max(1, n // 40))] = F(0.0)  # (a dark stratum: the floor decides)
    g = np.stack([delta, level], axis=1).astype(F)
    g[n // 3] = (np.inf, np.inf)
    g[(2 * n) // 3] = (np.nan, 1.0)
    return g


# ----- sanity of the restatements ------------------------------------------------------------------------------------
def test_strata_cover_the_frame_once_and_clamp():
    for (w, h), s in (((37, 21), 3), ((37, 21), 8), ((40, 24), 1), ((40, 24), 8), ((5, 3), 8)):
        sw, sh = -(-w // s), -(-h // s)
        for off in ((0, 0), (s - 1, s - 1)):
            pix = strata_pixels(w, h, s, off)
            assert len(pix) == sw * sh and len(np.unique(pix)) == sw * sh and pix.max() < w * h
            y, x = np.divmod(pix.astype(np.int64), w)
            assert np.array_equal(x // s, np.tile(np.arange(sw), sh)) and np.array_equal(y // s, np.repeat(np.arange(sh), sw))
        if w % s:  # the last column's pixel is clamped to the frame's last one
            assert strata_pixels(w, h, s, (s - 1, s - 1))[sw - 1] % w == w - 1
    assert np.array_equal(strata_pixels(40, 24, 1, (0, 0)), np.arange(960))


def test_gradient_restatement():
    old = np.array([[0.5, 0.25, 0.125], [1.0, 2.0, 3.0], [0.0, 0.0, 0.0]], dtype=F)
    new = np.array([[0.5, 0.25, 0.125], [3.0, 2.0, 1.0], [0.25, 0.0, 0.5]], dtype=F)
    got = gradient_reference(old, new, 3, 1, 1)
    assert got["gradient"].tolist() == [[0.0, 0.875], [4.0, 8.0], [0.75, 0.75]]
    assert got["resample"][:, :3].tobytes() == new.tobytes() and np.all(got["resample"][:, 3] == 1)
    assert got["pixel"].tolist() == [0, 1, 2]
    assert mean_color([np.array([[4096, 2048, 0]], dtype=np.uint32)] * 3).tolist() == [[1.0, 0.5, 0.0]]
    assert mean_color([np.full((1, 3), 0xffffffff, dtype=np.uint32)] * 2)[0, 0] == F(2.0 ** 32) * F(1.0 / 4096.0) / F(2.0)


def test_adapt_restatement():
    """λ = 1 gives length 0; the floor carries dark strata; a NaN or an inf in reach gives 0; and where every δ in reach is
    0 the length keeps its bits."""
    w, h, s = 37, 21, 3
    sw, sh = 13, 7
    lengths = np.random.default_rng(1).integers(0, 33, w * h).astype(F) + F(0.37)
    zero = np.zeros((sw * sh, 2), dtype=F)
    zero[:, 1] = 0.8
    assert adapt_reference(zero, lengths, w, h, s).tobytes() == lengths.tobytes()
    one = zero.copy()
    one[3 * sw + 5] = (0.9, 0.8)  # stratum (5, 3): pixels x 15..17, y 9..11
    got = adapt_reference(one, lengths, w, h, s, radius=1).reshape(h, w)
    reach = np.zeros((h, w), dtype=bool)
    reach[6:15, 12:21] = True
    assert got[~reach].tobytes() == lengths.reshape(h, w)[~reach].tobytes() and np.all(got[reach] < lengths.reshape(h, w)[reach])
    # D / M = 0.9 / (9 · 0.8) in the interior: f = (1 − q)^4
    M = F(0.0)
    for _ in range(9):
        M = F(M + F(0.8))
    q = F(0.9) / M
    keep = F(1.0) - q
    assert got[10, 16] == lengths.reshape(h, w)[10, 16] * (((keep * keep) * keep) * keep)
    for power, want in ((1, keep), (2, keep * keep)):
        assert adapt_reference(one, lengths, w, h, s, power=power).reshape(h, w)[10, 16] == lengths.reshape(h, w)[10, 16] * want
    assert np.all(adapt_reference(one, lengths, w, h, s, radius=0).reshape(h, w)[9:12, 15:18] == 0)  # q = 1.125: λ = 1
    assert np.all(adapt_reference(one, lengths, w, h, s, radius=0, gain=0.5).reshape(h, w)[9:12, 15:18] > 0)
    dark = np.zeros((sw * sh, 2), dtype=F)
    dark[0] = (0.001, 0.001)  # below the floor: q = 0.001 / 0.01
    assert adapt_reference(dark, lengths, w, h, s, radius=0, power=1)[0] == lengths[0] * (F(1.0) - F(0.001) / (F(0.01) * F(1.0)))
    for poison in ((np.nan, 1.0), (np.inf, np.inf), (np.inf, 1.0), (1.0, np.nan)):
        bad = zero.copy()
        bad[3 * sw + 5] = poison
        got = adapt_reference(bad, lengths, w, h, s).reshape(h, w)
        assert np.all(got[reach] == 0) and got[~reach].tobytes() == lengths.reshape(h, w)[~reach].tobytes(), poison
    g = synthetic_gradient(sw, sh, 5)
    got = adapt_reference(g, lengths, w, h, s)
    assert np.all(np.isfinite(got)) and (got == lengths).any() and (got == 0).mean() > 0.05 and len(np.unique(got / lengths)) > 10


# ---------------------------------------------------------------------------------------------------------------------
# The premise
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["c2_40x24", "c5"])
def test_premise_an_edit_changes_a_subset_of_the_pixels(name):
    """Sample 0 of the frame traced again after one sphere moved by +0.3 in x: δ > 0 in strictly between 5 % and 60 % of
    the strata at stride 1, an exact 0 elsewhere."""
    w, h = FRAMES[name][2]
    got = gradient_reference(mean_color([sample_reference(name, 0)[0]]), mean_color([edited_reference(name, 0)]), w, h, 1)
    share = float((got["gradient"][:, 0] > 0).mean())
    print(f"{name}: strata with a non-zero gradient {share:.4f}")
    assert 0.05 < share < 0.60
    same = got["gradient"][:, 0] == 0
    assert np.array_equal(sample_reference(name, 0)[0][same], edited_reference(name, 0)[same])


@pytest.mark.parametrize("name", list(EDITS))
def test_premise_both_oracles_agree_on_the_edited_scenes(name):
    """The geometric closest hit and the reference BVH's give the same samples on every pixel of the edited frames, so
    the GPU comparison may demand every stratum bit for bit; and the edit shows."""
    for s in range(SAMPLES):
        assert np.array_equal(edited_reference(name, s), edited_reference(name, s, exact=False)), (name, s)
    assert np.any(edited_reference(name, 0) != sample_reference(name, 0)[0])


# ---------------------------------------------------------------------------------------------------------------------
# The C ABI
# ---------------------------------------------------------------------------------------------------------------------
def test_structs_match_the_header():
    _check_layout("rt_temporal_gradient_args", abi.TemporalGradientArgs, 192)
    _check_layout("rt_history_adapt_args", abi.HistoryAdaptArgs, 72)
    assert [f[1] for f in _header_fields("rt_temporal_gradient_args")][:6] == ["prev_color", "gradient", "resample", "pixel",
                                                                              "counters", "rng_seed"]
    assert [f[1] for f in _header_fields("rt_history_adapt_args")][:2] == ["gradient", "history"]
    assert abi.TemporalGradientArgs.reserved.size == 12 and abi.HistoryAdaptArgs.reserved.size == 8


def test_exports_and_abi_version():
    for name in ("rt_temporal_gradient", "rt_history_adapt"):
        assert name in EXPORTED
        assert hasattr(lib(), name)
    assert lib().rt_abi_version() == 14 and abi.ABI_VERSION == 14  # (additions that change no layout)
    assert "#define RT_ABI_VERSION 14" in HEADER
    comment = HEADER[:HEADER.index("#define RT_ABI_VERSION")]
    comment = comment[comment.rindex("/*"):]
    assert "rt_temporal_gradient" in comment and "rt_history_adapt" in comment
    assert "XORWOW" in HEADER[HEADER.index("Re-trace and compare"):HEADER.index("typedef struct rt_temporal_gradient_args")]


# ----- rt_temporal_gradient ------------------------------------------------------------------------------------------
W, H, STRIDE = 16, 8, 3  # 6 x 3 strata
STRATA = 18
GRADIENT_BUFFERS = ("prev_color", "gradient", "resample", "pixel", "counters")
GRADIENT_BYTES = {"prev_color": W * H * 16, "gradient": STRATA * 8, "resample": STRATA * 16, "pixel": STRATA * 4,
                  "counters": abi.COUNTERS_WORDS * 8}


def _gradient_args(w: int = W, h: int = H):
    """Valid arguments over host dummies (never dereferenced: every check precedes the first device call)."""
    arena = C.create_string_buffer(len(GRADIENT_BUFFERS) * SLOT)
    a = abi.TemporalGradientArgs()
    for k, name in enumerate(GRADIENT_BUFFERS):
        setattr(a, name, C.addressof(arena) + k * SLOT)
    a.width, a.height, a.stride, a.offset_x, a.offset_y = w, h, STRIDE, 1, 2
    a.samples_per_pixel, a.max_depth, a.rng_seed, a.rng_frame = 1, 8, SEED, 3
    a.tiling = abi.Tiling(max(h, 1), 1, 0, h)
    a.inputs = scenes.CONFIGS["c2"].inputs()
    return a, arena


def _bogus_scene():
    return C.cast(C.create_string_buffer(64), C.c_void_p)  # never dereferenced: the arguments are checked first


def test_gradient_rejects_bad_arguments():
    L, scene, who = lib(), _bogus_scene(), "rt_temporal_gradient"
    call = lambda a, s=scene: L.rt_temporal_gradient(s, C.byref(a), None)  # noqa: E731
    _rejected(L.rt_temporal_gradient(scene, None, None), who, "NULL args")
    a, keep = _gradient_args()
    _rejected(call(a, None), who, "NULL scene")
    for name in ("prev_color", "gradient"):
        a, keep = _gradient_args()
        setattr(a, name, None)
        _rejected(call(a), who, "NULL " + name)
    for field, values in (("stride", (0, 9, 0xffffffff)), ("offset_x", (3, 8, 0xffffffff)), ("offset_y", (3, 0xffffffff)),
                          ("samples_per_pixel", (0, 17, 0xffffffff)), ("rays_per_lane", (17, 0xffffffff)),
                          ("count_tests", (2, 1 << 31)),
                          ("flags", (1, 2, 4, 16, abi.RT_FLAG_RNG_PHILOX, 1 << 31, abi.RT_FLAG_RIUS_LEFT_TO_RIGHT | 1))):
        for bad in values:
            a, keep = _gradient_args()
            setattr(a, field, bad)
            _rejected(call(a), who, field)
    a, keep = _gradient_args()
    a.stride, a.offset_x, a.offset_y = 1, 1, 0  # (an offset is below the stride, whatever the stride)
    _rejected(call(a), who, "offset_x")
    a, keep = _gradient_args()
    a.count_tests, a.counters = 1, None
    _rejected(call(a), who, "without counters")
    for k in range(3):
        a, keep = _gradient_args()
        a.reserved[k] = 1
        _rejected(call(a), who, "reserved")
    a, keep = _gradient_args()
    a.tiling = abi.Tiling(4, 2, 0, 4)
    _rejected(call(a), who, "num_ranks")
    a, keep = _gradient_args()
    a.tiling = abi.Tiling(H, 1, 0, H - 1)
    _rejected(call(a), who, "local_rows")
    a, keep = _gradient_args()
    a.width, a.height = 0x10000, 0x8000  # 2^31 pixels
    a.tiling = abi.Tiling(0x8000, 1, 0, 0x8000)
    _rejected(call(a), who, "too large")
    # valid: the limits, the optional outputs left out, depth 0, the fill-order flag (a NULL scene stops the call)
    a, keep = _gradient_args()
    a.stride, a.offset_x, a.offset_y, a.samples_per_pixel, a.rays_per_lane, a.count_tests = 8, 7, 7, 16, 16, 1
    a.flags, a.max_depth, a.resample, a.pixel = abi.RT_FLAG_RIUS_LEFT_TO_RIGHT, 0, None, None
    _rejected(call(a, None), who, "NULL scene")
    a, keep = _gradient_args()
    a.counters, a.tiling = None, abi.Tiling(H, 1, 0, 0)
    _rejected(call(a, None), who, "NULL scene")


def test_gradient_rejects_overlapping_buffers():
    L, scene, who = lib(), _bogus_scene(), "rt_temporal_gradient"
    for n, first in enumerate(GRADIENT_BUFFERS):
        for second in GRADIENT_BUFFERS[n + 1:]:
            for shift in (0, GRADIENT_BYTES[first] - 1):
                a, keep = _gradient_args()
                setattr(a, second, getattr(a, first) + shift)
                _rejected(L.rt_temporal_gradient(scene, C.byref(a), None), who, f"{second} overlaps {first}")
    a, keep = _gradient_args()
    a.resample = a.gradient + STRATA * 8  # adjacent, not overlapping
    _rejected(L.rt_temporal_gradient(None, C.byref(a), None), who, "NULL scene")


def test_gradient_empty_frame_is_accepted_without_a_device():
    for w, h in ((0, H), (W, 0), (0, 0)):
        a, keep = _gradient_args(w, h)
        assert lib().rt_temporal_gradient(None, C.byref(a), None) == 0
        for name in GRADIENT_BUFFERS:
            setattr(a, name, None)
        assert lib().rt_temporal_gradient(None, C.byref(a), None) == 0
        a.flags = 1  # ... but the arguments are still checked
        _rejected(lib().rt_temporal_gradient(None, C.byref(a), None), "rt_temporal_gradient", "flags")
        a.flags, a.stride = 0, 0
        _rejected(lib().rt_temporal_gradient(None, C.byref(a), None), "rt_temporal_gradient", "stride")


# ----- rt_history_adapt ----------------------------------------------------------------------------------------------
def _adapt_args(w: int = W, h: int = H):
    arena = C.create_string_buffer(2 * SLOT)
    a = abi.HistoryAdaptArgs()
    a.gradient, a.history = C.addressof(arena), C.addressof(arena) + SLOT
    a.width, a.height, a.stride, a.radius, a.power, a.gain, a.lum_floor = w, h, STRIDE, 1, 4, 1.0, 0.01
    a.tiling = abi.Tiling(max(h, 1), 1, 0, h)
    return a, arena


def test_adapt_rejects_bad_arguments():
    L, who = lib(), "rt_history_adapt"
    call = lambda a: L.rt_history_adapt(C.byref(a), None)  # noqa: E731
    _rejected(L.rt_history_adapt(None, None), who, "NULL args")
    for name in ("gradient", "history"):
        a, keep = _adapt_args()
        setattr(a, name, None)
        _rejected(call(a), who, "NULL " + name)
    for field, values in (("stride", (0, 9, 0xffffffff)), ("radius", (4, 0xffffffff)), ("power", (0, 9, 0xffffffff)),
                          ("gain", (0.0, -1.0, float("nan"))), ("lum_floor", (0.0, -0.5, float("nan"))),
                          ("flags", (1, 1 << 31))):
        for bad in values:
            a, keep = _adapt_args()
            setattr(a, field, bad)
            _rejected(call(a), who, field)
    for k in range(2):
        a, keep = _adapt_args()
        a.reserved[k] = 1
        _rejected(call(a), who, "reserved")
    a, keep = _adapt_args()
    a.tiling = abi.Tiling(4, 2, 0, 4)
    _rejected(call(a), who, "num_ranks")
    a, keep = _adapt_args()
    a.tiling = abi.Tiling(H, 1, 0, H - 1)
    _rejected(call(a), who, "local_rows")
    a, keep = _adapt_args()
    a.width, a.height = 0x10000, 0x8000
    a.tiling = abi.Tiling(0x8000, 1, 0, 0x8000)
    _rejected(call(a), who, "too large")
    # the gradient plane must not overlap the history plane: its first and last byte against either end
    for shift in (0, W * H * 16 - 1):
        a, keep = _adapt_args()
        a.gradient = a.history + shift
        _rejected(call(a), who, "gradient overlaps history")
    a, keep = _adapt_args()
    a.history = a.gradient + STRATA * 8 - 1
    _rejected(call(a), who, "gradient overlaps history")


def test_adapt_empty_frame_is_accepted_without_a_device():
    for w, h in ((0, H), (W, 0), (0, 0)):
        a, keep = _adapt_args(w, h)
        assert lib().rt_history_adapt(C.byref(a), None) == 0
        a.gradient = a.history = None
        assert lib().rt_history_adapt(C.byref(a), None) == 0
        a.flags = 1  # ... but the arguments are still checked
        _rejected(lib().rt_history_adapt(C.byref(a), None), "rt_history_adapt", "flags")
        a.flags, a.power = 0, 0
        _rejected(lib().rt_history_adapt(C.byref(a), None), "rt_history_adapt", "power")


# ---------------------------------------------------------------------------------------------------------------------
# Quality: the history's error after an edit
# ---------------------------------------------------------------------------------------------------------------------
PRE, POST, MAX_HISTORY, REFERENCE_SPP = 32, 6, 32, 512
SETTINGS = dict(stride=3, radius=1, power=4, gain=1.0, lum_floor=0.01)
# halfway between the adapted value measured and the better alternative: (0.00731 + 0.01146) / 2, (0.00628 + 0.01180) / 2
QUALITY_BOUNDS = {"c2_ground_frame1_whole": 0.00939, "c5_move_frame6_changed": 0.00904}


def _frame(scene: scenes.Scene, name: str, k: int, spp: int = 1) -> np.ndarray:
    """Philox frame k of `scene` under the frame's camera: (W·H, 3) float32, the radiance plane's rgb."""
    _, _, (w, h), depth = FRAMES[name]
    acc = np.zeros(w * h * 4, dtype=F)
    po.render(po.OracleScene(scene, exact=True), w, h, spp, depth, frame_inputs(name), None, philox=True, seed=SEED, frame=k,
              accum=acc, rius_order=1, threads=8)
    return (acc.reshape(w * h, 4)[:, :3] / F(spp)).astype(F)


def _blend(hist: np.ndarray, length: np.ndarray, c: np.ndarray) -> tuple:
    """Step 5 of rt_temporal for a resting camera, in float32."""
    N = np.minimum((length + F(1.0)).astype(F), F(MAX_HISTORY)).astype(F)
    alpha = (F(1.0) / N).astype(F)
    return (hist + (alpha[:, None] * (c - hist).astype(F)).astype(F)).astype(F), N


@functools.lru_cache(maxsize=None)
def after_edit(name: str, what: str) -> dict:
    """{variant: [(whole-frame MSE, changed-pixel MSE) for each of the POST frames after the edit]} for "plain" (the
    lengths as they are), "reset" (all 0) and "adapted" (rt_history_adapt's, from the gradient of the last frame before
    the edit at SETTINGS, the stratum offset the PRE-th call of a rotating caller has)."""
    edit = {"ground": recolor(0, (0.8, 0.2, 0.2)), "wall": recolor(0, (0.1, 0.1, 0.9)), "move2": move(2, 0.3)}[what]
    w, h = FRAMES[name][2]
    A = frame_scene(name)
    B = edited(A, edit)
    ref = _frame(B, name, 1000, REFERENCE_SPP)
    changed = np.abs(ref - _frame(A, name, 1000, REFERENCE_SPP)).sum(axis=1) > 0.1
    hist, length = None, None
    for k in range(PRE):
        c = _frame(A, name, k)
        hist, length = (c.copy(), np.ones(w * h, dtype=F)) if hist is None else _blend(hist, length, c)
    s = SETTINGS["stride"]
    turn = (PRE - 1) % (s * s)
    g = gradient_reference(_frame(A, name, PRE - 1), _frame(B, name, PRE - 1), w, h, s, (turn % s, turn // s))
    starts = {"plain": length, "reset": np.zeros_like(length),
              "adapted": adapt_reference(g["gradient"], length, w, h, **SETTINGS)}
    fresh = [_frame(B, name, k) for k in range(PRE, PRE + POST)]
    out = {"changed_share": float(changed.mean()), "gradient_share": float((g["gradient"][:, 0] > 0).mean())}
    for variant, n in starts.items():
        hv, errs = hist, []
        for c in fresh:
            hv, n = _blend(hv, n, c)
            e = ((hv - ref).astype(np.float64) ** 2)
            errs.append((float(e.mean()), float(e[changed].mean()) if changed.any() else 0.0))
        out[variant] = errs
    return out


def _report(name: str, what: str, r: dict) -> None:
    print(f"{name} {what}: changed pixels {r['changed_share']:.3f}, strata with a gradient {r['gradient_share']:.3f}")
    for variant in ("plain", "reset", "adapted"):
        print(f"  {variant:8s}", " ".join(f"{e:.5f}/{a:.4f}" for e, a in r[variant]))


def test_quality_c2_ground_recoloured():
    """Frame 1 after the edit, whole frame: the adapted history's error is below both plain continuation and a full
    reset.  Measured: adapted 0.00731, plain 0.01146, reset 0.01203; the bound lies halfway between the adapted value
    and the better alternative."""
    r = after_edit("c2_40x24", "ground")
    _report("c2_40x24", "ground recoloured", r)
    adapted, plain, reset = r["adapted"][0][0], r["plain"][0][0], r["reset"][0][0]
    assert adapted < plain and adapted < reset
    assert adapted < QUALITY_BOUNDS["c2_ground_frame1_whole"]


def test_quality_c5_sphere_moved():
    """Frame 6 after the edit, on the pixels whose converged colour changed by more than 0.1: the adapted history's error
    is below plain continuation's.  Measured: adapted 0.00628, plain 0.01180 (a full reset: 0.0052); the bound lies halfway."""
    r = after_edit("c5", "move2")
    _report("c5", "sphere 2 moved", r)
    adapted, plain = r["adapted"][POST - 1][1], r["plain"][POST - 1][1]
    assert adapted < plain
    assert adapted < QUALITY_BOUNDS["c5_move_frame6_changed"]


def test_quality_c3_is_reported():
    """A box lit by a small emitter: its 1-spp frames are mostly fireflies, a few changed firefly paths carry a huge
    difference and drop their neighbourhood's history, and the pass loses to plain continuation (DESIGN.md §19 lists it
    as a limit).  Measured at frame 1, whole frame: adapted 0.1102, plain 0.0447, reset 1.485.  Computed and printed;
    nothing is asserted about the errors."""
    r = after_edit("c3", "wall")
    _report("c3", "a wall recoloured", r)
    assert set(r) >= {"plain", "reset", "adapted"}
