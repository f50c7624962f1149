"""rt_adaptive_select and rt_adaptive_samples without a device: the structs against the header, the exports, every
argument check, and the numpy restatements that tests/test_gpu_adaptive.py compares the kernels with.

select_reference restates the selection rule of include/rt_hip.h in float32, one rounding per operation: only
multiplications, additions and comparisons, so the kernel's k must equal it bit for bit.  merge_history and merge_accum
restate the merge of rt_adaptive_samples (step 5 of rt_temporal / rt_temporal_moments for a resting camera, and
RT_FLAG_ACCUMULATE's addition) on samples given in 2^-12 units, which is what tests/test_radiance_host.py
sample_reference returns for the oracle."""
from __future__ import annotations

import ctypes as C

import numpy as np
import pytest

from cudaraytracer_amd import abi, scenes
from cudaraytracer_amd._lib import EXPORTED, lib

from test_radiance_host import HEADER, _check_layout, _header_fields, _rejected

F = np.float32
SLOT = 1 << 16  # bytes between the dummy buffers of the argument tests (the largest, a 16 x 8 float4 plane: 2048)


# ---------------------------------------------------------------------------------------------------------------------
# The numpy restatements
# ---------------------------------------------------------------------------------------------------------------------
def select_k(history_w, moments, prim_id, tau, lum_floor, min_history, max_samples) -> np.ndarray:
    """k(p) of rt_adaptive_select_args for flat planes: history_w (n,), moments (n, 2), prim_id (n,) or None."""
    w = np.asarray(history_w, dtype=F)
    m1, m2 = np.asarray(moments, dtype=F)[:, 0], np.asarray(moments, dtype=F)[:, 1]
    with np.errstate(invalid="ignore", over="ignore"):
        N = np.where(w > F(1.0), w, F(1.0)).astype(F)
        d = (m2 - (m1 * m1).astype(F)).astype(F)
        v = np.where(d > F(0.0), d, F(0.0)).astype(F)
        m = np.where(m1 > F(lum_floor), m1, F(lum_floor)).astype(F)
        T = (F(F(tau) * F(tau)) * (m * m).astype(F)).astype(F)
        k = np.zeros(w.shape, dtype=np.uint32)
        for j in range(max_samples):
            Nj = (N + F(j)).astype(F)
            k += ((Nj < F(min_history)) | (v > (Nj * T).astype(F))).astype(np.uint32)
    if prim_id is not None:
        k[np.asarray(prim_id) < 0] = 0
    return k


def select_reference(history_w, moments, prim_id, tau, lum_floor, min_history, max_samples) -> tuple:
    """(pixels, samples, count): the whole list in ascending pixel order and count = (listed pixels, their k summed)."""
    k = select_k(history_w, moments, prim_id, tau, lum_floor, min_history, max_samples)
    pixels = np.nonzero(k)[0].astype(np.uint32)
    return pixels, k[pixels], np.array([len(pixels), int(k.sum())], dtype=np.uint32)


def luminance(c: np.ndarray) -> np.ndarray:
    """rt_temporal_moments' luminance of (n, 3) float32 colours."""
    return ((F(0.2126) * c[:, 0] + F(0.7152) * c[:, 1]).astype(F) + F(0.0722) * c[:, 2]).astype(F)


def merge_history(history, moments, units, max_history) -> tuple:
    """history (n, 4) and moments (n, 2) after one more sample per pixel, `units` (n, 3) in 2^-12 units: step 5 of
    rt_temporal_moments for a resting camera, in float32."""
    h, mo = np.array(history, dtype=F), np.array(moments, dtype=F)
    c = (units.astype(F) * F(1.0 / 4096.0)).astype(F)
    N = np.minimum((h[:, 3] + F(1.0)).astype(F), F(max_history)).astype(F)
    alpha = (F(1.0) / N).astype(F)
    for ch in range(3):
        h[:, ch] = (h[:, ch] + (alpha * (c[:, ch] - h[:, ch]).astype(F)).astype(F)).astype(F)
    h[:, 3] = N
    lum = luminance(c)
    mo[:, 0] = (mo[:, 0] + (alpha * (lum - mo[:, 0]).astype(F)).astype(F)).astype(F)
    mo[:, 1] = (mo[:, 1] + (alpha * ((lum * lum).astype(F) - mo[:, 1]).astype(F)).astype(F)).astype(F)
    return h, mo


def reset_planes(units) -> tuple:
    """(history, moments) as a reset pass of rt_temporal_moments leaves them for a frame of these samples: (c, 1),
    (l, l·l)."""
    c = (units.astype(F) * F(1.0 / 4096.0)).astype(F)
    lum = luminance(c)
    return (np.concatenate([c, np.ones((len(c), 1), dtype=F)], axis=1),
            np.stack([lum, (lum * lum).astype(F)], axis=1).astype(F))


def merge_accum(accum, unit_sum, k) -> np.ndarray:
    """accum (n, 4) after adding an entry's k samples whose 2^-12 units sum to unit_sum (n, 3): one float add per
    channel, w += k."""
    out = np.array(accum, dtype=F)
    s = (np.minimum(unit_sum.astype(np.uint64), np.uint64(0xffffffff)).astype(F) * F(1.0 / 4096.0)).astype(F)
    out[:, :3] = (out[:, :3] + s).astype(F)
    out[:, 3] = (out[:, 3] + np.asarray(k).astype(F)).astype(F)
    return out


def synthetic_planes(w: int, h: int, seed: int, miss_share: float = 0.3) -> tuple:
    """Planes of a w x h frame for the selection: gamma-distributed moments, history lengths 0..40 with non-integers
    among them, and about miss_share misses.  (history (n, 4), moments (n, 2), prim_id (n,) int32)"""
    rng = np.random.default_rng(seed)
    n = w * h
    m1 = rng.gamma(2.0, 0.25, n).astype(F)
    spread = rng.gamma(1.5, 0.05, n).astype(F)
    m2 = (m1 * m1 + spread * rng.integers(0, 2, n).astype(F)).astype(F)  # (about half have no variance to speak of)
    length = rng.integers(0, 41, n).astype(F)
    odd = rng.random(n) < 0.25
    length[odd] = (length[odd] + rng.random(odd.sum()).astype(F)).astype(F)
    history = np.concatenate([rng.random((n, 3)).astype(F), length[:, None]], axis=1).astype(F)
    prim_id = np.where(rng.random(n) < miss_share, -1, rng.integers(0, 500, n)).astype(np.int32)
    return history, np.stack([m1, m2], axis=1).astype(F), prim_id


# ----- sanity of the restatement -------------------------------------------------------------------------------------
PARAMS = dict(tau=0.15, lum_floor=0.01, min_history=4, max_samples=8)


def test_rule_is_zero_on_a_miss_and_a_prefix_count():
    hist, mom, pid = synthetic_planes(65, 33, 1)
    k = select_k(hist[:, 3], mom, pid, **PARAMS)
    assert np.all(k[pid < 0] == 0) and 0.05 < (k > 0).mean() < 0.9 and k.max() == PARAMS["max_samples"]
    assert len(np.unique(k)) > 3
    # a prefix: the predicate of sample j holds exactly for j < k — so a smaller cap only cuts the count
    for cap in (1, 2, 5):
        assert np.array_equal(select_k(hist[:, 3], mom, pid, **{**PARAMS, "max_samples": cap}), np.minimum(k, cap))
    pixels, samples, count = select_reference(hist[:, 3], mom, pid, **PARAMS)
    assert np.all(np.diff(pixels.astype(np.int64)) > 0) and np.array_equal(samples, k[pixels])
    assert count[0] == len(pixels) == (k > 0).sum() and count[1] == k.sum()
    # without prim_id every pixel is valid
    assert (select_k(hist[:, 3], mom, None, **PARAMS) > 0).sum() > count[0]


def test_rule_raising_tau_never_raises_k():
    hist, mom, pid = synthetic_planes(40, 24, 2)
    last = None
    for tau in (0.02, 0.05, 0.1, 0.3, 1.0, 1e6):
        k = select_k(hist[:, 3], mom, pid, **{**PARAMS, "tau": tau})
        if last is not None:
            assert np.all(k <= last)
        last = k
    assert last.max() == 3  # min_history = 4 alone is left: at most 3 more after N = 1


def test_rule_min_history_alone():
    """With no variance, k = min(max_samples, ceil(min_history − N)) for integer N (N = max(w, 1))."""
    w = np.arange(0, 30, dtype=F)
    mom = np.stack([np.full(30, 0.5, dtype=F), np.full(30, 0.25, dtype=F)], axis=1)
    for min_history in (0, 1, 4, 17):
        for cap in (1, 3, 16):
            k = select_k(w, mom, None, tau=0.1, lum_floor=0.01, min_history=min_history, max_samples=cap)
            want = np.clip(min_history - np.maximum(w, 1), 0, cap).astype(np.uint32)
            assert np.array_equal(k, want), (min_history, cap)
    # NaNs compare false: no variance term; the history term is N = 1's
    mom[:, 1] = np.nan
    assert np.array_equal(select_k(w, mom, None, 0.1, 0.01, 0, 16), np.zeros(30, dtype=np.uint32))
    assert np.all(select_k(np.full(30, np.nan, dtype=F), mom, None, 0.1, 0.01, 4, 16) == 3)


def test_merge_restatements():
    """One merged sample is rt_temporal_moments' blend; k samples saturate the way the render's sums do."""
    rng = np.random.default_rng(3)
    units = rng.integers(0, 1 << 14, (50, 3)).astype(np.uint32)
    h0, m0 = reset_planes(units)
    assert np.all(h0[:, 3] == 1) and np.array_equal(m0[:, 1], (m0[:, 0] * m0[:, 0]).astype(F))
    h1, m1 = merge_history(h0, m0, units, 32)  # the same sample again: the mean stays, N = 2
    assert np.all(h1[:, 3] == 2) and np.array_equal(h1[:, :3], h0[:, :3]) and np.array_equal(m1, m0)
    h2, _ = merge_history(h1, m1, units, 2)  # the cap: N stays 2, alpha 1/2
    assert np.all(h2[:, 3] == 2)
    acc = merge_accum(np.zeros((50, 4), dtype=F), units.astype(np.uint64) * 2, 2)
    assert np.all(acc[:, 3] == 2) and np.array_equal(acc[:, :3], (units * 2).astype(F) / F(4096.0))


# ---------------------------------------------------------------------------------------------------------------------
# The C ABI
# ---------------------------------------------------------------------------------------------------------------------
def test_structs_match_the_header():
    _check_layout("rt_adaptive_select_args", abi.AdaptiveSelectArgs, 120)
    _check_layout("rt_adaptive_samples_args", abi.AdaptiveSamplesArgs, 192)
    assert [f[1] for f in _header_fields("rt_adaptive_select_args")][:7] == ["history", "moments", "prim_id", "pixels", "samples",
                                                                            "count", "scratch"]
    assert [f[1] for f in _header_fields("rt_adaptive_samples_args")][:7] == ["pixels", "samples", "count", "history", "moments",
                                                                             "accum", "counters"]
    assert abi.AdaptiveSelectArgs.reserved.size == 12 and abi.AdaptiveSamplesArgs.reserved.size == 8


def test_exports_and_abi_version():
    for name in ("rt_adaptive_select", "rt_adaptive_select_scratch_bytes", "rt_adaptive_samples"):
        assert name in EXPORTED
        assert hasattr(lib(), name)
    assert lib().rt_abi_version() == 14 and abi.ABI_VERSION == 14  # (additions that change no layout)
    assert "#define RT_ABI_VERSION 14" in HEADER
    comment = HEADER[:HEADER.index("#define RT_ABI_VERSION")]
    comment = comment[comment.rindex("/*"):]
    assert "rt_adaptive_select" in comment and "rt_adaptive_samples" in comment


def test_scratch_bytes():
    sb = lib().rt_adaptive_select_scratch_bytes
    assert sb(0, 5) == 0 and sb(7, 0) == 0
    assert sb(1, 1) == 8 and sb(16, 16) == 8 and sb(257, 1) == 16 and sb(1920, 1080) == 8100 * 8
    assert sb(0xffffffff, 0xffffffff) > 1 << 50  # (64-bit arithmetic)


# ----- rt_adaptive_select --------------------------------------------------------------------------------------------
W, H = 16, 8
SELECT_BUFFERS = ("history", "moments", "prim_id", "pixels", "samples", "count", "scratch")
SELECT_BYTES = {"history": W * H * 16, "moments": W * H * 8, "prim_id": W * H * 4, "pixels": 64 * 4, "samples": 64 * 4, "count": 8,
                "scratch": 8}


def _select_args(capacity: int = 64, w: int = W, h: int = H):
    """Valid arguments over host dummies (never dereferenced: every check precedes the first device call)."""
    arena = C.create_string_buffer(len(SELECT_BUFFERS) * SLOT)
    a = abi.AdaptiveSelectArgs()
    for k, name in enumerate(SELECT_BUFFERS):
        setattr(a, name, C.addressof(arena) + k * SLOT)
    a.width, a.height, a.capacity = w, h, capacity
    a.max_samples, a.min_history, a.tau, a.lum_floor = 4, 4, 0.1, 0.01
    a.tiling = abi.Tiling(h, 1, 0, h)
    return a, arena


def test_select_rejects_bad_arguments():
    L, who = lib(), "rt_adaptive_select"
    call = lambda a: L.rt_adaptive_select(C.byref(a), None)  # noqa: E731
    _rejected(L.rt_adaptive_select(None, None), who, "NULL args")
    for name in ("history", "moments", "pixels", "count", "scratch"):
        a, keep = _select_args()
        setattr(a, name, None)
        _rejected(call(a), who, "NULL " + name)
    for field, values in (("tau", (0.0, -1.0, float("nan"))), ("lum_floor", (0.0, -0.5, float("nan"))),
                          ("min_history", (4097, 0xffffffff)), ("max_samples", (0, 17, 0xffffffff)),
                          ("pixels_per_lane", (17, 0xffffffff)), ("flags", (1, 1 << 31))):
        for bad in values:
            a, keep = _select_args()
            setattr(a, field, bad)
            _rejected(call(a), who, field)
    for k in range(3):
        a, keep = _select_args()
        a.reserved[k] = 1
        _rejected(call(a), who, "reserved")
    a, keep = _select_args()
    a.tiling = abi.Tiling(4, 2, 0, 4)
    _rejected(call(a), who, "num_ranks")
    a, keep = _select_args()
    a.tiling = abi.Tiling(H, 1, 0, H - 1)
    _rejected(call(a), who, "local_rows")
    a, keep = _select_args()
    a.width, a.height = 0x10000, 0x8000  # 2^31 pixels
    a.tiling = abi.Tiling(0x8000, 1, 0, 0x8000)
    _rejected(call(a), who, "too large")
    a, keep = _select_args()
    a.width, a.height, a.max_samples = 0x10000, 0x1000, 16  # 2^28 pixels of up to 16 samples: the sum needs 33 bits
    a.tiling = abi.Tiling(0x1000, 1, 0, 0x1000)
    _rejected(call(a), who, "too large")
    a, keep = _select_args()
    a.scratch += 2
    _rejected(call(a), who, "aligned")


def test_select_rejects_overlapping_buffers():
    """An output may share no byte with an input or with another output; the message names both."""
    L, who = lib(), "rt_adaptive_select"
    outs, ins = ("pixels", "samples", "count", "scratch"), ("history", "moments", "prim_id")
    for o in outs:
        for i in ins:
            for shift in (0, SELECT_BYTES[i] - (4 if o == "scratch" else 1)):  # the input's first and last byte (word)
                a, keep = _select_args()
                setattr(a, o, getattr(a, i) + shift)
                _rejected(L.rt_adaptive_select(C.byref(a), None), who, f"{o} overlaps {i}")
    for n, first in enumerate(outs):
        for second in outs[n + 1:]:
            for shift in (0, SELECT_BYTES[first] - (4 if second == "scratch" else 1)):
                a, keep = _select_args()
                setattr(a, second, getattr(a, first) + shift)
                _rejected(L.rt_adaptive_select(C.byref(a), None), who, f"{second} overlaps {first}")


def test_select_empty_frame_is_accepted_without_a_device():
    for w, h in ((0, H), (W, 0), (0, 0)):
        a, keep = _select_args(w=w, h=h)
        a.count = None  # (with count the call clears it on the device)
        assert lib().rt_adaptive_select(C.byref(a), None) == 0
        for name in SELECT_BUFFERS:
            setattr(a, name, None)
        assert lib().rt_adaptive_select(C.byref(a), None) == 0
        a.flags = 1  # ... but the arguments are still checked
        _rejected(lib().rt_adaptive_select(C.byref(a), None), "rt_adaptive_select", "flags")
        a.flags, a.tau = 0, 0.0
        _rejected(lib().rt_adaptive_select(C.byref(a), None), "rt_adaptive_select", "tau")


# ----- rt_adaptive_samples -------------------------------------------------------------------------------------------
SAMPLES_BUFFERS = ("pixels", "samples", "count", "counters", "history", "moments", "accum")
SAMPLES_BYTES = {"pixels": 64 * 4, "samples": 64 * 4, "count": 4, "counters": abi.COUNTERS_WORDS * 8, "history": W * H * 16,
                 "moments": W * H * 8, "accum": W * H * 16}


def _samples_args(capacity: int = 64):
    arena = C.create_string_buffer(len(SAMPLES_BUFFERS) * SLOT)
    a = abi.AdaptiveSamplesArgs()
    for k, name in enumerate(SAMPLES_BUFFERS):
        setattr(a, name, C.addressof(arena) + k * SLOT)
    a.capacity, a.width, a.height = capacity, W, H
    a.samples_per_pixel, a.max_samples, a.sample_base, a.max_depth, a.max_history = 1, 4, 1, 8, 32
    a.inputs = scenes.CONFIGS["c2"].inputs()
    return a, arena


def _bogus_scene():
    return C.cast(C.create_string_buffer(64), C.c_void_p)  # never dereferenced: the arguments are checked first


def test_samples_rejects_bad_arguments():
    L, scene, who = lib(), _bogus_scene(), "rt_adaptive_samples"
    call = lambda a, s=scene: L.rt_adaptive_samples(s, C.byref(a), None)  # noqa: E731
    _rejected(L.rt_adaptive_samples(scene, None, None), who, "NULL args")
    a, keep = _samples_args()
    _rejected(call(a, None), who, "NULL scene")
    a, keep = _samples_args()
    a.pixels = None
    _rejected(call(a), who, "NULL pixels")
    a, keep = _samples_args()
    a.history = a.moments = a.accum = None
    _rejected(call(a), who, "no target")
    for accum in (True, False):
        a, keep = _samples_args()
        a.history = None
        if not accum:
            a.accum = None
        _rejected(call(a), who, "moments without history")
    for field, values in (("rays_per_lane", (17, 0xffffffff)), ("count_tests", (2, 1 << 31)),
                          ("max_samples", (0, 17, 0xffffffff)), ("max_history", (0, 4097, 0xffffffff)),
                          ("flags", (1, 2, 4, 16, abi.RT_FLAG_RNG_PHILOX, 1 << 31, abi.RT_FLAG_RIUS_LEFT_TO_RIGHT | 1))):
        for bad in values:
            a, keep = _samples_args()
            setattr(a, field, bad)
            _rejected(call(a), who, field)
    a, keep = _samples_args()
    a.count_tests, a.counters = 1, None
    _rejected(call(a), who, "without counters")
    for k in range(2):
        a, keep = _samples_args()
        a.reserved[k] = 1
        _rejected(call(a), who, "reserved")
    a, keep = _samples_args()
    a.samples, a.samples_per_pixel = None, 0
    _rejected(call(a), who, "samples_per_pixel")
    for base, cap in ((abi.PHILOX_MAX_SPP, 1), (abi.PHILOX_MAX_SPP - 3, 4), (0xffffffff, 16)):
        a, keep = _samples_args()
        a.sample_base, a.max_samples = base, cap
        _rejected(call(a), who, "RT_PHILOX_MAX_SPP")
    a, keep = _samples_args()
    a.width, a.height = 0x10000, 0x8000
    _rejected(call(a), who, "too large")
    for w, h in ((0, H), (W, 0)):
        a, keep = _samples_args()
        a.width, a.height = w, h
        _rejected(call(a), who, "empty frame")
    # valid: the limits, each target alone, no count, no samples, the fill-order flag (a NULL scene stops the call)
    a, keep = _samples_args()
    a.sample_base, a.max_samples, a.max_history, a.rays_per_lane, a.count_tests = abi.PHILOX_MAX_SPP - 16, 16, 4096, 16, 1
    a.flags, a.count, a.samples, a.max_depth = abi.RT_FLAG_RIUS_LEFT_TO_RIGHT, None, None, 0
    _rejected(call(a, None), who, "NULL scene")
    for keep_only in (("history",), ("accum",), ("history", "moments")):
        a, keep = _samples_args()
        for name in ("history", "moments", "accum"):
            if name not in keep_only:
                setattr(a, name, None)
        _rejected(call(a, None), who, "NULL scene")


def test_samples_rejects_overlapping_buffers():
    L, scene, who = lib(), _bogus_scene(), "rt_adaptive_samples"
    for n, first in enumerate(SAMPLES_BUFFERS):
        for second in SAMPLES_BUFFERS[n + 1:]:
            for shift in (0, SAMPLES_BYTES[first] - 1):
                a, keep = _samples_args()
                setattr(a, second, getattr(a, first) + shift)
                _rejected(L.rt_adaptive_samples(scene, C.byref(a), None), who, f"{second} overlaps {first}")
    a, keep = _samples_args()
    a.moments = a.history + W * H * 16  # adjacent, not overlapping
    _rejected(L.rt_adaptive_samples(None, C.byref(a), None), who, "NULL scene")


def test_samples_empty_list_is_accepted_without_a_device():
    a, keep = _samples_args(0)
    assert lib().rt_adaptive_samples(None, C.byref(a), None) == 0
    a.pixels = None
    a.width = a.height = 0
    assert lib().rt_adaptive_samples(None, C.byref(a), None) == 0
    a.flags = 1  # ... but the arguments are still checked
    _rejected(lib().rt_adaptive_samples(None, C.byref(a), None), "rt_adaptive_samples", "flags")
    a.flags, a.history, a.accum = 0, None, None
    _rejected(lib().rt_adaptive_samples(None, C.byref(a), None), "rt_adaptive_samples", "moments without history")
