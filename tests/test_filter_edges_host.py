"""The frames, offsets and parameter sweeps of tests/test_gpu_filter_edges.py, and the properties of the numpy definitions
(test_denoise_host.py filter_reference, test_variance_host.py variance_filter_reference) those GPU tests stand on.

The embedding property.  Both filters skip a tap outside the frame and a tap on a miss pixel (prim_id < 0) the same way:
its weight becomes 0, and sw + 0, 0·finite + s and a row never visited all leave the sums' bits alone.  Iteration i of a
pixel is the same arithmetic wherever the pixel lies, its taps in row-major order.  So the result on a set of planes is
bit for bit the crop of the result on the same planes placed anywhere in a larger frame whose surround is miss pixels
with finite values (`embed`).  Pinned here for the float32 numpy definitions, which are exact restatements of the order
of operations; the GPU module asserts it of the kernels, where it checks tile staging, halos and frame clipping at every
tile alignment without any tolerance.

The other tests pin what the GPU module's tolerances need: every edge frame's float64 reference is finite, and every one
with at least four hit pixels has a non-zero float32-vs-float64 spread d on rgb (frames of fewer pixels have d = 0 or a
few 1e-8, which is why the edge-frame bound has a floor: test_gpu_filter_edges.py)."""
from __future__ import annotations

import functools

import numpy as np
import pytest

from cudaraytracer_amd import abi

from test_denoise_host import filter_reference, synthetic_planes
from test_variance_host import VARIANCE_DEFAULTS, variance_filter_reference, variance_planes

F = np.float32

CONTENT = (37, 29)          # (width, height) of synthetic_planes / variance_planes
FRAME = (96, 64)            # the frame CONTENT is embedded in: 3 x 4 tiles of 32 x 16
OFFSETS = ((0, 0), (1, 1), (27, 3), (31, 15), (32, 16), (59, 35))  # (ox, oy) of CONTENT in FRAME
# (27, 3): tile (1, 1) lies wholly under the content; (32, 16): the content's corner on a tile corner; the others make the
# content straddle every tile edge, (59, 35) with its far corner on the frame's
EDGE_SHAPES = ((1, 1), (1, 40), (40, 1), (2, 2), (3, 3), (31, 15), (32, 16), (33, 17), (64, 32), (65, 33))
SHAPE_FRAME = (112, 64)     # holds every edge shape at both SHAPE_OFFSETS with surround on every side
SHAPE_OFFSETS = ((32, 16), (27, 3))

DENOISE_SIGMAS = (0.6, 0.1, 0.05)  # sigma_c, sigma_n, sigma_z: rt_denoise's defaults
BOTH_FLAGS = abi.RT_DENOISE_DEMODULATE | abi.RT_DENOISE_COLOR_IS_SUM
DENOISE_FLAGS = (0, BOTH_FLAGS)
# one parameter at a time away from the defaults, far below and far above
DENOISE_SWEEPS = (("sigma_c", 0.02), ("sigma_c", 50.0), ("sigma_n", 0.01), ("sigma_n", 10.0), ("sigma_z", 0.005),
                  ("sigma_z", 5.0))
# (history lengths are 1..8: min_history 1 = every pixel takes its own moments, 9 = every pixel the 7x7 estimate)
VARIANCE_SWEEPS = (("sigma_l", 0.05), ("sigma_l", 20.0), ("min_history", 1), ("min_history", 9))
SWEEP_ITERATIONS = 3

SURROUND = {"color": (0.3, 0.3, 0.3, 1.0), "accum": (0.3, 0.3, 0.3, 1.0), "normal_depth": (0.0, 0.0, 0.0, -1.0),
            "albedo": (1.0, 1.0, 1.0, 1.0), "prim_id": -1, "moments": (0.0, 0.0)}


def embed(planes: dict, width: int, height: int, ox: int, oy: int) -> dict:
    """The planes at (ox, oy) of a width x height frame of miss pixels with finite values (SURROUND).  Read-only."""
    out = {}
    for key, fill in SURROUND.items():
        if key not in planes:
            continue
        src = planes[key]
        h, w = src.shape[:2]
        assert 0 <= ox and ox + w <= width and 0 <= oy and oy + h <= height
        a = np.empty((height, width) + src.shape[2:], dtype=src.dtype)
        a[...] = fill
        a[oy:oy + h, ox:ox + w] = src
        a.setflags(write=False)
        out[key] = a
    return out


def crop(a: np.ndarray, width: int, height: int, ox: int, oy: int) -> np.ndarray:
    return np.ascontiguousarray(a[oy:oy + height, ox:ox + width])


def denoise_sigmas(name: str | None = None, value: float | None = None) -> tuple:
    s = dict(zip(("sigma_c", "sigma_n", "sigma_z"), DENOISE_SIGMAS))
    if name is not None:
        assert name in s
        s[name] = value
    return tuple(s.values())


@functools.lru_cache(maxsize=None)
def denoise_planes(width: int = CONTENT[0], height: int = CONTENT[1], ox: int | None = None, oy: int = 0,
                   frame: tuple = FRAME) -> dict:
    """synthetic_planes(width, height), embedded at (ox, oy) of `frame` unless ox is None.  Read-only, computed once."""
    p = synthetic_planes(width, height)
    for a in p.values():
        a.setflags(write=False)
    return p if ox is None else embed(p, frame[0], frame[1], ox, oy)


@functools.lru_cache(maxsize=None)
def filter_planes(width: int = CONTENT[0], height: int = CONTENT[1], ox: int | None = None, oy: int = 0,
                  frame: tuple = FRAME) -> dict:
    """variance_planes(width, height), likewise."""
    p = {k: v for k, v in variance_planes(width, height).items() if isinstance(v, np.ndarray)}
    return p if ox is None else embed(p, frame[0], frame[1], ox, oy)


def denoise_reference(p: dict, iterations: int, flags: int, sigmas: tuple, dtype) -> np.ndarray:
    color = p["accum"] if flags & abi.RT_DENOISE_COLOR_IS_SUM else p["color"]
    return filter_reference(color, p["normal_depth"], p["albedo"], p["prim_id"], iterations, *sigmas, flags, dtype=dtype)


def variance_reference(p: dict, iterations: int, params: dict, dtype) -> np.ndarray:
    kw = dict(VARIANCE_DEFAULTS, iterations=iterations, **params)
    return variance_filter_reference(p["color"], p["moments"], p["normal_depth"], p["prim_id"], **kw, dtype=dtype)


@functools.lru_cache(maxsize=None)
def denoise_references(key: tuple, iterations: int, flags: int = 0, sigmas: tuple = DENOISE_SIGMAS) -> tuple:
    """(float64, float32) runs of rt_denoise's definition on denoise_planes(*key); computed once, shared."""
    p = denoise_planes(*key)
    return tuple(denoise_reference(p, iterations, flags, sigmas, t) for t in (np.float64, np.float32))


@functools.lru_cache(maxsize=None)
def variance_references(key: tuple, iterations: int, params: tuple = ()) -> tuple:
    """(float64, float32) runs of rt_denoise_variance's definition on filter_planes(*key); params: ((name, value), ...)."""
    p = filter_planes(*key)
    return tuple(variance_reference(p, iterations, dict(params), t) for t in (np.float64, np.float32))


def spread(r64: np.ndarray, r32: np.ndarray, channels) -> float:
    """d of the GPU tests: the largest difference between the definition's float32 and float64 runs."""
    return float(np.abs(r32[channels].astype(np.float64) - r64[channels]).max())


RGB, VAR = np.s_[..., :3], np.s_[..., 3]


def hit_pixels(width: int, height: int) -> int:
    return int((denoise_planes(width, height)["prim_id"] >= 0).sum())


# ---------------------------------------------------------------------------------------------------------------------
# embed itself
# ---------------------------------------------------------------------------------------------------------------------
def test_embed_places_the_planes_in_a_frame_of_misses():
    for planes in (denoise_planes(), filter_planes()):
        e = embed(planes, *FRAME, 27, 3)
        assert set(e) == set(planes)
        inside = np.zeros(FRAME[::-1], dtype=bool)
        inside[3:3 + CONTENT[1], 27:27 + CONTENT[0]] = True
        for key, a in e.items():
            assert a.dtype == planes[key].dtype and a.shape == FRAME[::-1] + planes[key].shape[2:]
            assert crop(a, *CONTENT, 27, 3).tobytes() == planes[key].tobytes()
            assert np.isfinite(a).all()
            assert np.all(a[~inside] == np.asarray(SURROUND[key], dtype=a.dtype)), key
        assert np.all(e["prim_id"][~inside] == -1)
    # the offsets put an interior tile under the content, its corner on a tile corner, and it across every tile edge
    assert (27 <= 32 and 27 + CONTENT[0] >= 64) and (3 <= 16 and 3 + CONTENT[1] >= 32)
    assert all(ox + CONTENT[0] <= FRAME[0] and oy + CONTENT[1] <= FRAME[1] for ox, oy in OFFSETS)
    for w, h in EDGE_SHAPES:
        for ox, oy in SHAPE_OFFSETS:
            assert ox >= 1 and oy >= 1 and ox + w < SHAPE_FRAME[0] and oy + h < SHAPE_FRAME[1]


# ---------------------------------------------------------------------------------------------------------------------
# The float32 definitions are bit-invariant under embedding
# ---------------------------------------------------------------------------------------------------------------------
def _assert_invariant(width, height, ox, oy, frame, iterations) -> None:
    plain, inner = denoise_planes(width, height), denoise_planes(width, height, ox, oy, frame)
    for flags in DENOISE_FLAGS:
        a = denoise_reference(plain, iterations, flags, DENOISE_SIGMAS, F)
        b = crop(denoise_reference(inner, iterations, flags, DENOISE_SIGMAS, F), width, height, ox, oy)
        assert a.tobytes() == b.tobytes(), ("rt_denoise", flags, int((a != b).any(-1).sum()))
    plain, inner = filter_planes(width, height), filter_planes(width, height, ox, oy, frame)
    a = variance_reference(plain, iterations, {}, F)
    b = crop(variance_reference(inner, iterations, {}, F), width, height, ox, oy)
    assert a.tobytes() == b.tobytes(), ("rt_denoise_variance", int((a != b).any(-1).sum()))


@pytest.mark.parametrize("iterations", [3, 6])
@pytest.mark.parametrize("offset", OFFSETS, ids=lambda o: f"at{o[0]}_{o[1]}")
def test_definitions_are_bit_invariant_under_embedding(offset, iterations):
    _assert_invariant(*CONTENT, *offset, FRAME, iterations)


@pytest.mark.parametrize("iterations", [3, 6])
@pytest.mark.parametrize("shape", EDGE_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_edge_shapes_are_bit_invariant_under_embedding(shape, iterations):
    for ox, oy in SHAPE_OFFSETS:
        _assert_invariant(*shape, ox, oy, SHAPE_FRAME, iterations)


# ---------------------------------------------------------------------------------------------------------------------
# What the GPU module's tolerances rest on
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", EDGE_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_edge_shape_references_are_finite_with_a_spread(shape):
    n = filter_planes(*shape)["color"][..., 3]
    hits = hit_pixels(*shape)
    for iterations in (1, 6):
        for label, (r64, r32) in (("rt_denoise", denoise_references(shape, iterations)),
                                  ("rt_denoise_variance", variance_references(shape, iterations))):
            assert r64.dtype == np.float64 and np.isfinite(r64).all() and np.isfinite(r32).all(), label
            d = spread(r64, r32, RGB)
            print(f"{shape[0]}x{shape[1]} N={iterations} {label}: {hits} hit pixels, d rgb {d:.3e}, max |r64| "
                  f"{np.abs(r64[RGB]).max():.3f}")
            if hits >= 4:
                assert d > 0, label
    if hits >= 4:
        assert (n < VARIANCE_DEFAULTS["min_history"]).any() and (n >= VARIANCE_DEFAULTS["min_history"]).any()


def test_sweeps_move_one_parameter_each_and_have_a_spread():
    assert {n for n, _ in DENOISE_SWEEPS} == {"sigma_c", "sigma_n", "sigma_z"}
    assert {n for n, _ in VARIANCE_SWEEPS} == {"sigma_l", "min_history"}
    key = CONTENT
    base = denoise_references(key, SWEEP_ITERATIONS)[0]
    for name, value in DENOISE_SWEEPS:
        sig = denoise_sigmas(name, value)
        assert sum(a != b for a, b in zip(sig, DENOISE_SIGMAS)) == 1
        r64, r32 = denoise_references(key, SWEEP_ITERATIONS, 0, sig)
        assert np.isfinite(r64).all() and spread(r64, r32, RGB) > 0 and not np.array_equal(r64, base), (name, value)
    n = filter_planes()["color"][..., 3]
    assert n.min() == 1 and n.max() == 8  # so min_history 1 and 9 put every hit pixel on one side
    base = variance_references(key, SWEEP_ITERATIONS)[0]
    for name, value in VARIANCE_SWEEPS:
        r64, r32 = variance_references(key, SWEEP_ITERATIONS, ((name, value),))
        assert np.isfinite(r64).all() and not np.array_equal(r64, base), (name, value)
        assert spread(r64, r32, RGB) > 0 and spread(r64, r32, VAR) > 0, (name, value)
