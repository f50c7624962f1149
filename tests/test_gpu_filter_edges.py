"""rt_denoise and rt_denoise_variance on the GPU in every launch form, at every tile alignment and at the frame's edges
(frames, offsets and sweeps: tests/test_filter_edges_host.py; runners: test_gpu_denoise.py, test_gpu_variance.py).

Launch forms.  Iteration i of an N-iteration call runs denoise_kernel<S, FIRST, LAST> / dnv_kernel<S, LAST> with
S = 1, 2, 4 for i = 0, 1, 2 and the global-memory build S = 0 from i = 3 on; LAST is i = N - 1.  N = 1 .. 6 therefore
runs each of the eight forms of either template as a last launch (N = 1, 2, 3 and 4..6) and as an inner one, with the
global build at steps 8, 16 and 32; dnv_variance_kernel runs in every rt_denoise_variance call.

Tolerances, three kinds:
  * against the definition (tests a, c): the rule of test_gpu_denoise.py / test_gpu_variance.py, unchanged.  d = the
    largest absolute difference between the numpy definition's own float32 and float64 runs on the case; the kernel may
    order a sum differently, contract a multiply-add or use another exponential, each worth about one such spread, so
    err <= 4·d, on rgb and on the variance channel each with its own d, and d > 0 is asserted;
  * the edge frames of test c only: 4·max(d, 2^-24·max|r64|).  A frame of a few pixels has one to four taps per pixel
    and d measures almost nothing there (0 at 1x1, ~5e-8 at 2x2: test_filter_edges_host.py prints them), while the
    kernel still rounds w·c and the quotient sum / sw once each.  The floor is half a float32 ulp of the largest output
    value, one rounding of the result; it is derived, not fitted, and applies to that list alone;
  * none (tests b, d and the w = 1 case): embedding invariance, guard regions and the exact division compare bits.

Embedding invariance (test b).  A tap outside the frame and a tap on a miss are skipped the same way — the weight is
selected to 0.0f, and sw + 0, fma(0, finite, s) and a skipped row leave the sums alone — iteration i of a pixel is the same
template form wherever the pixel lies, and the LDS and the global build sum their taps in the same row-major order.  So
the output on a set of planes equals, bit for bit on every pixel, the crop of the output on the same planes placed at
any offset of a larger frame of finite miss pixels.  Any halo, staging, clipping or indexing mistake at some tile
alignment breaks it, however small its numeric effect.

Measured on MI355X (every test prints its figures; tables in DESIGN.md §11, §14): rt_denoise N = 1..6 error / d 1.00 ..
1.11, its sweeps 0.76 .. 1.14; rt_denoise_variance N = 1..6 1.14 .. 1.69 (rgb) and 1.06 .. 1.87 (variance), its sweeps
0.60 .. 1.93; edge frames error / bound 0.00 .. 0.45.  Every bit-for-bit comparison holds, miss pixels included."""
from __future__ import annotations

import ctypes as C
import functools

import numpy as np
import pytest
import torch

from cudaraytracer_amd import abi
from cudaraytracer_amd._lib import lib

from test_denoise_host import rgb_to_int_np
from test_filter_edges_host import (BOTH_FLAGS, CONTENT, DENOISE_FLAGS, DENOISE_SIGMAS, DENOISE_SWEEPS, EDGE_SHAPES, FRAME,
                                    OFFSETS, RGB, SHAPE_FRAME, SHAPE_OFFSETS, SWEEP_ITERATIONS, VAR, VARIANCE_SWEEPS,
                                    crop, denoise_planes, denoise_references, denoise_sigmas, filter_planes, spread,
                                    variance_references)
from test_gpu_denoise import run_denoise
from test_gpu_variance import run_variance
from test_variance_host import VARIANCE_DEFAULTS

pytestmark = pytest.mark.gpu

FILL = -7.0              # sentinel of the float guards
POS_FILL = 0x5A5A5A5A    # ... and of pos's
GUARD = 3                # rows (of the frame's width) before and after each output and the scratch
INTERIOR = (27, 3)       # the offset of FRAME at which tile (1, 1) has full neighbours on all four sides
FILTERS = ("denoise", "denoise_both_flags", "variance")


def shape_id(s) -> str:
    return f"{s[0]}x{s[1]}"


def offset_id(o) -> str:
    return f"at{o[0]}_{o[1]}"


@functools.lru_cache(maxsize=None)
def gpu_run(which: str, key: tuple, iterations: int) -> tuple:
    """(out_color, pos) of one call at the defaults on denoise_planes(*key) / filter_planes(*key); once per process."""
    if which == "variance":
        out, pos = run_variance(filter_planes(*key), iterations)
    else:
        out, pos = run_denoise(denoise_planes(*key), iterations, BOTH_FLAGS if which == "denoise_both_flags" else 0,
                               DENOISE_SIGMAS)
    out.setflags(write=False)
    pos.setflags(write=False)
    return out, pos


def check_against(label: str, out: np.ndarray, pos: np.ndarray, refs: tuple, channels, floor: bool = False) -> None:
    """err <= 4·d per channel group (floor: 4·max(d, 2^-24·max|r64|)), pos = the epilogue of the kernel's own out_color."""
    r64, r32 = refs
    assert np.isfinite(out).all()
    for name, sl in channels:
        d = spread(r64, r32, sl)
        err = float(np.abs(out[sl].astype(np.float64) - r64[sl]).max())
        bound = 4 * d
        if floor:
            half_ulp = 2.0 ** -24 * float(np.abs(r64[sl]).max())
            bound = 4 * max(d, half_ulp)
            print(f"{label} {name}: GPU error {err:.3e}, d {d:.3e}, floor {half_ulp:.3e}, error / bound {err / bound if bound else 0.0:.2f}")
        else:
            print(f"{label} {name}: GPU error {err:.3e}, float32-vs-float64 spread d {d:.3e}, ratio {err / d if d else float('inf'):.2f}")
            assert d > 0, (label, name)
        assert err <= bound, (label, name, err, d)
    assert np.array_equal(pos, rgb_to_int_np(out[RGB]))


DENOISE_CHANNELS = (("rgb", RGB),)
VARIANCE_CHANNELS = (("rgb", RGB), ("variance", VAR))


# ---------------------------------------------------------------------------------------------------------------------
# a. Every launch form against the definition
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("flags", DENOISE_FLAGS)
@pytest.mark.parametrize("iterations", [1, 2, 3, 4, 5, 6])
def test_denoise_every_form_matches_the_definition(iterations, flags):
    """37x29: N = 1..6 end in <1,true,true>, <2,false,true>, <4,false,true> and <0,false,true> at steps 8, 16, 32."""
    which = "denoise_both_flags" if flags else "denoise"
    out, pos = gpu_run(which, CONTENT, iterations)
    check_against(f"rt_denoise 37x29 N={iterations} flags={flags}", out, pos, denoise_references(CONTENT, iterations, flags),
                  DENOISE_CHANNELS)
    assert np.all(out[..., 3] == 1.0)


@pytest.mark.parametrize("iterations", [1, 2, 3, 4, 5, 6])
def test_variance_every_form_matches_the_definition(iterations):
    out, pos = gpu_run("variance", CONTENT, iterations)
    check_against(f"rt_denoise_variance 37x29 N={iterations}", out, pos, variance_references(CONTENT, iterations),
                  VARIANCE_CHANNELS)
    assert np.all(out[..., 3] >= 0)


@pytest.mark.parametrize("which", FILTERS)
@pytest.mark.parametrize("iterations", [2, 4, 6])
def test_interior_tiles_match_the_definition(iterations, which):
    """The planes at (27, 3) of 96x64: tile (1, 1) has full neighbours, so its halo is staged whole from four sides."""
    key = CONTENT + INTERIOR
    out, pos = gpu_run(which, key, iterations)
    if which == "variance":
        refs, channels = variance_references(key, iterations), VARIANCE_CHANNELS
    else:
        refs, channels = denoise_references(key, iterations, BOTH_FLAGS if which == "denoise_both_flags" else 0), DENOISE_CHANNELS
    check_against(f"{which} 37x29 at (27,3) of 96x64 N={iterations}", out, pos, refs, channels)


# ---------------------------------------------------------------------------------------------------------------------
# b. Embedding invariance, bit for bit
# ---------------------------------------------------------------------------------------------------------------------
def assert_crop_is_the_plain_run(which: str, shape: tuple, offset: tuple, frame: tuple, iterations: int) -> None:
    plain_out, plain_pos = gpu_run(which, shape, iterations)
    out, pos = gpu_run(which, shape + offset + (frame,), iterations)
    got_out, got_pos = crop(out, *shape, *offset), crop(pos, *shape, *offset)
    if got_out.tobytes() != plain_out.tobytes() or got_pos.tobytes() != plain_pos.tobytes():
        bad = (got_out.view(np.uint32) != plain_out.view(np.uint32)).any(-1) | (got_pos != plain_pos)
        ys, xs = np.nonzero(bad)
        hit = denoise_planes(*shape)["prim_id"] >= 0
        pytest.fail(f"{which} {shape_id(shape)} N={iterations} at {offset} of {shape_id(frame)}: {len(ys)} pixels differ "
                    f"({int((bad & hit).sum())} hits, {int((bad & ~hit).sum())} misses), first (x, y) = ({xs[0]}, {ys[0]}): "
                    f"{got_out[ys[0], xs[0]]} vs plain {plain_out[ys[0], xs[0]]}; columns {sorted(set(xs.tolist()))[:12]}, "
                    f"rows {sorted(set(ys.tolist()))[:12]}")


@pytest.mark.parametrize("which", FILTERS)
@pytest.mark.parametrize("iterations", [1, 2, 3, 4, 6])
@pytest.mark.parametrize("offset", OFFSETS, ids=offset_id)
def test_the_output_does_not_depend_on_the_tile_alignment(offset, iterations, which):
    """out_color (all four channels) and pos of the 37x29 planes embedded at `offset` of 96x64, cropped = the plain run."""
    assert_crop_is_the_plain_run(which, CONTENT, offset, FRAME, iterations)


@pytest.mark.parametrize("which", FILTERS)
@pytest.mark.parametrize("shape", EDGE_SHAPES, ids=shape_id)
def test_frame_edge_clipping_is_the_miss_skipping(shape, which):
    """Frames smaller than the windows, single rows and columns, tile boundaries +-1: the frame's own edge (clipping)
    against the same pixels surrounded by misses (skipping), at a tile corner and across tile edges; N = 1, 3, 6."""
    for iterations in (1, 3, 6):
        for offset in SHAPE_OFFSETS:
            assert_crop_is_the_plain_run(which, shape, offset, SHAPE_FRAME, iterations)


# ---------------------------------------------------------------------------------------------------------------------
# c. Edge shapes and parameter sweeps against the definition
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("iterations", [1, 6])
@pytest.mark.parametrize("shape", EDGE_SHAPES, ids=shape_id)
def test_edge_shapes_match_the_definition(shape, iterations):
    out, pos = gpu_run("denoise", shape, iterations)
    check_against(f"rt_denoise {shape_id(shape)} N={iterations}", out, pos, denoise_references(shape, iterations),
                  DENOISE_CHANNELS, floor=True)
    out, pos = gpu_run("variance", shape, iterations)
    check_against(f"rt_denoise_variance {shape_id(shape)} N={iterations}", out, pos, variance_references(shape, iterations),
                  VARIANCE_CHANNELS, floor=True)


@pytest.mark.parametrize("name,value", DENOISE_SWEEPS)
def test_denoise_parameter_sweep(name, value):
    """One of sigma_c, sigma_n, sigma_z far from its default: the constants k_c, k_n, k_z folded on the host / per pixel
    and v_exp_f32 over the range of arguments they produce."""
    sig = denoise_sigmas(name, value)
    out, pos = run_denoise(denoise_planes(), SWEEP_ITERATIONS, 0, sig)
    check_against(f"rt_denoise {name}={value}", out, pos, denoise_references(CONTENT, SWEEP_ITERATIONS, 0, sig), DENOISE_CHANNELS)


@pytest.mark.parametrize("name,value", VARIANCE_SWEEPS)
def test_variance_parameter_sweep(name, value):
    """sigma_l far from its default (k_l), and min_history 1 / 9: with history lengths 1..8 every pixel takes its own
    moments / every pixel takes the 7x7 estimate."""
    out, pos = run_variance(filter_planes(), SWEEP_ITERATIONS, **{name: value})
    check_against(f"rt_denoise_variance {name}={value}", out, pos,
                  variance_references(CONTENT, SWEEP_ITERATIONS, ((name, value),)), VARIANCE_CHANNELS)


@pytest.mark.parametrize("iterations", [1, 4])
def test_color_is_sum_with_unit_weights_is_the_plain_colour(iterations):
    """RT_DENOISE_COLOR_IS_SUM on a plane whose w is 1 everywhere: x / 1 is exact, so the bits of the plain run."""
    p = denoise_planes()
    assert np.all(p["color"][..., 3] == 1.0)
    want = gpu_run("denoise", CONTENT, iterations)
    out, pos = run_denoise(dict(p, accum=p["color"]), iterations, abi.RT_DENOISE_COLOR_IS_SUM, DENOISE_SIGMAS)
    assert out.tobytes() == want[0].tobytes() and pos.tobytes() == want[1].tobytes()


# ---------------------------------------------------------------------------------------------------------------------
# d. Nothing is written outside what the API reports
# ---------------------------------------------------------------------------------------------------------------------
def run_guarded(which: str, planes: dict, iterations: int) -> dict:
    """One call whose out_color, pos and scratch lie between GUARD rows of sentinel; the scratch is exactly the reported
    byte count.  Returns the three buffers whole and the input planes as the device holds them afterwards."""
    dev = torch.device("cuda", 0)
    h, w = planes["prim_id"].shape
    variance = which == "variance"
    names = ("color", "moments", "normal_depth", "prim_id") if variance else ("color", "normal_depth", "albedo", "prim_id")
    t = {k: torch.from_numpy(np.array(planes[k])).to(dev) for k in names}
    sizer = lib().rt_denoise_variance_scratch_bytes if variance else lib().rt_denoise_scratch_bytes
    need = int(sizer(w, h, iterations))
    assert need == w * h * 16 * ((1 if iterations <= 1 else 2) if variance else min(iterations - 1, 2))
    g = GUARD * w
    out = torch.full(((h + 2 * GUARD) * w, 4), FILL, dtype=torch.float32, device=dev)
    pos = torch.full(((h + 2 * GUARD) * w,), POS_FILL, dtype=torch.int32, device=dev)
    scratch = torch.full((2 * g + need // 16, 4), FILL, dtype=torch.float32, device=dev)
    a = abi.DenoiseVarianceArgs() if variance else abi.DenoiseArgs()
    for k, v in t.items():
        setattr(a, k, v.data_ptr())
    a.out_color, a.pos, a.scratch = out[g:].data_ptr(), pos[g:].data_ptr(), scratch[g:].data_ptr()
    a.width, a.height, a.iterations = w, h, iterations
    a.tiling = abi.Tiling(h, 1, 0, h)
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    if variance:
        a.min_history = VARIANCE_DEFAULTS["min_history"]
        a.sigma_l, a.sigma_n, a.sigma_z = (VARIANCE_DEFAULTS[k] for k in ("sigma_l", "sigma_n", "sigma_z"))
        rc = lib().rt_denoise_variance(C.byref(a), stream)
    else:
        a.flags = abi.RT_DENOISE_DEMODULATE
        a.sigma_c, a.sigma_n, a.sigma_z = DENOISE_SIGMAS
        rc = lib().rt_denoise(C.byref(a), stream)
    assert rc == 0, lib().rt_last_error()
    torch.cuda.synchronize()
    return {"out": out.cpu().numpy(), "pos": pos.cpu().numpy(), "scratch": scratch.cpu().numpy(), "need": need,
            "inputs": {k: v.cpu().numpy() for k, v in t.items()}}


@pytest.mark.parametrize("which", ["denoise", "variance"])
@pytest.mark.parametrize("iterations", [1, 2, 3])
@pytest.mark.parametrize("shape", [(33, 17), (65, 33)], ids=shape_id)
def test_nothing_is_written_outside_the_reported_sizes(shape, iterations, which):
    """Partial tiles on the right and below (one column, one row).  N = 1, 2, 3: scratch of 0, 1, 2 planes (rt_denoise;
    N = 1 gets a pointer into the guards and must not use it) and 1, 2, 2 planes (rt_denoise_variance)."""
    w, h = shape
    planes = filter_planes(*shape) if which == "variance" else denoise_planes(*shape)
    got = run_guarded(which, planes, iterations)
    g, n = GUARD * w, w * h
    assert np.all(got["out"][:g] == FILL) and np.all(got["out"][g + n:] == FILL)
    assert np.all(got["pos"][:g] == POS_FILL) and np.all(got["pos"][g + n:] == POS_FILL)
    s = got["scratch"]
    assert s.shape[0] == 2 * g + got["need"] // 16
    assert np.all(s[:g] == FILL) and np.all(s[g + got["need"] // 16:] == FILL)
    assert not np.any(s[g:g + got["need"] // 16, :3] == FILL)  # (every reported plane is used: rgb of each pixel written)
    for k, v in got["inputs"].items():
        assert v.tobytes() == planes[k].tobytes(), k
    out, pos = got["out"][g:g + n].reshape(h, w, 4), got["pos"][g:g + n].view(np.uint32).reshape(h, w)
    assert np.isfinite(out).all() and np.array_equal(pos, rgb_to_int_np(out[RGB]))
    if which == "variance":
        want = gpu_run("variance", shape, iterations)
        assert out.tobytes() == want[0].tobytes() and pos.tobytes() == want[1].tobytes()
