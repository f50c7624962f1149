"""rt_denoise on the GPU against the numpy restatement of its definition (tests/test_denoise_host.py filter_reference).

Tolerance of the filter comparison: d = the largest absolute difference between the reference's own float32 and float64
runs on the same inputs; the kernel may sum its 25 terms in another order and use another expf, each worth about one
such spread, so 4·d is allowed.  Measured on MI355X over the twelve cases: d = 3.5e-7 .. 7.4e-7, GPU error between
0.83·d and 1.11·d."""
from __future__ import annotations

import ctypes as C
import functools

import numpy as np
import pytest
import torch

from cudaraytracer_amd import abi
from cudaraytracer_amd._lib import lib
from cudaraytracer_amd.renderer import DeviceScene, Renderer

from test_denoise_host import (E2E_SIZE, end_to_end_frame, filter_reference, mse, rgb_to_int_np, synthetic_planes)

pytestmark = pytest.mark.gpu

SIGMAS = (0.6, 0.1, 0.05)


def run_denoise(planes: dict, iterations: int, flags: int, sigmas=SIGMAS, want_pos: bool = True,
                want_out: bool = True) -> tuple:
    """(out_color (H, W, 4) float32, pos (H, W) uint32) of one rt_denoise call on the planes (numpy, host)."""
    dev = torch.device("cuda", 0)
    h, w = planes["prim_id"].shape
    color = planes["accum"] if flags & abi.RT_DENOISE_COLOR_IS_SUM else planes["color"]
    t = {k: torch.from_numpy(np.array(v)).to(dev) for k, v in
         (("color", color), ("nd", planes["normal_depth"]), ("albedo", planes["albedo"]), ("prim", planes["prim_id"]))}
    out = torch.full((h, w, 4), -7.0, dtype=torch.float32, device=dev)
    pos = torch.zeros((h, w), dtype=torch.int32, device=dev)
    need = int(lib().rt_denoise_scratch_bytes(w, h, iterations))
    scratch = torch.zeros(max(need, 1), dtype=torch.uint8, device=dev)
    a = abi.DenoiseArgs()
    a.color, a.normal_depth, a.albedo, a.prim_id = (t[k].data_ptr() for k in ("color", "nd", "albedo", "prim"))
    a.out_color = out.data_ptr() if want_out else None
    a.pos = pos.data_ptr() if want_pos else None
    a.scratch = scratch.data_ptr() if need else None
    a.width, a.height, a.iterations, a.flags = w, h, iterations, flags
    a.sigma_c, a.sigma_n, a.sigma_z = sigmas
    a.tiling = abi.Tiling(h, 1, 0, h)
    rc = lib().rt_denoise(C.byref(a), C.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0, lib().rt_last_error()
    torch.cuda.synchronize()
    return out.cpu().numpy(), pos.cpu().numpy().view(np.uint32)


@functools.lru_cache(maxsize=None)
def planes() -> dict:
    p = synthetic_planes()  # 37 x 29: smaller than the 2·16 reach of iteration 5, so borders clip
    for a in p.values():
        a.setflags(write=False)
    return p


@functools.lru_cache(maxsize=None)
def references(iterations: int, flags: int) -> tuple:
    p = planes()
    color = p["accum"] if flags & abi.RT_DENOISE_COLOR_IS_SUM else p["color"]
    args = (color, p["normal_depth"], p["albedo"], p["prim_id"], iterations) + SIGMAS + (flags,)
    return filter_reference(*args, dtype=np.float64), filter_reference(*args, dtype=np.float32)


@pytest.mark.parametrize("is_sum", [0, abi.RT_DENOISE_COLOR_IS_SUM])
@pytest.mark.parametrize("demodulate", [0, abi.RT_DENOISE_DEMODULATE])
@pytest.mark.parametrize("iterations", [1, 3, 5])
def test_filter_matches_the_reference(iterations, demodulate, is_sum):
    flags = demodulate | is_sum
    r64, r32 = references(iterations, flags)
    out, _ = run_denoise(planes(), iterations, flags)
    d = float(np.abs(r32.astype(np.float64) - r64).max())
    err = float(np.abs(out[..., :3].astype(np.float64) - r64).max())
    print(f"N={iterations} flags={flags}: GPU error {err:.3e}, float32-vs-float64 spread d {d:.3e}, ratio {err / d:.2f}")
    assert d > 0
    assert err <= 4 * d, (err, d)
    assert np.all(out[..., 3] == 1.0)


@pytest.mark.parametrize("iterations,flags", [(1, 0), (3, abi.RT_DENOISE_DEMODULATE), (5, abi.RT_DENOISE_COLOR_IS_SUM)])
def test_epilogue_is_the_render_kernels(iterations, flags):
    """pos = rgb_to_int(255·sqrtf(out_color)) bit for bit (Kernel.cu:12-19, 152-157), from the LDS and the global
    build's last launch alike."""
    out, pos = run_denoise(planes(), iterations, flags)
    assert np.array_equal(pos, rgb_to_int_np(out[..., :3]))


@pytest.mark.parametrize("iterations", [1, 2, 4])
def test_miss_pixels_pass_through(iterations):
    """prim_id < 0: c_{i+1}(p) = c_i(p), the same bits — the colour itself without demodulation, and with it the
    float32 value (colour / a) · a of the fused divide and multiply (a = max(albedo, 1/256))."""
    p = planes()
    miss = p["prim_id"] < 0
    out, _ = run_denoise(p, iterations, 0)
    assert out[..., :3][miss].tobytes() == p["color"][..., :3][miss].tobytes()
    out, _ = run_denoise(p, iterations, abi.RT_DENOISE_DEMODULATE)
    a = np.maximum(p["albedo"][..., :3], np.float32(1.0 / 256.0))
    want = (p["color"][..., :3] / a) * a
    assert out[..., :3][miss].tobytes() == want[miss].astype(np.float32).tobytes()


def test_out_color_aliasing_color_is_rejected():
    """include/rt_hip.h: out_color must not alias color; the call fails before any launch and writes nothing."""
    dev = torch.device("cuda", 0)
    p = planes()
    h, w = p["prim_id"].shape
    color = torch.from_numpy(np.array(p["color"])).to(dev)
    others = [torch.from_numpy(np.array(p[k])).to(dev) for k in ("normal_depth", "albedo", "prim_id")]
    scratch = torch.zeros(int(lib().rt_denoise_scratch_bytes(w, h, 3)), dtype=torch.uint8, device=dev)
    a = abi.DenoiseArgs()
    a.color = a.out_color = color.data_ptr()
    a.normal_depth, a.albedo, a.prim_id = (t.data_ptr() for t in others)
    a.scratch = scratch.data_ptr()
    a.width, a.height, a.iterations, a.flags = w, h, 3, 0
    a.sigma_c, a.sigma_n, a.sigma_z = SIGMAS
    a.tiling = abi.Tiling(h, 1, 0, h)
    assert lib().rt_denoise(C.byref(a), None) == -1
    assert b"alias" in lib().rt_last_error()
    torch.cuda.synchronize()
    assert np.array_equal(color.cpu().numpy(), p["color"])


def test_two_calls_give_the_same_bits():
    a = run_denoise(planes(), 5, abi.RT_DENOISE_DEMODULATE)
    b = run_denoise(planes(), 5, abi.RT_DENOISE_DEMODULATE)
    assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()


def test_each_output_is_optional():
    """The last launch writes out_color alone, the RGBA8 framebuffer alone, or both: the same values."""
    full = run_denoise(planes(), 3, abi.RT_DENOISE_DEMODULATE)
    out, pos = run_denoise(planes(), 3, abi.RT_DENOISE_DEMODULATE, want_out=False)
    assert np.array_equal(pos, full[1]) and np.all(out == -7.0)
    out, pos = run_denoise(planes(), 3, abi.RT_DENOISE_DEMODULATE, want_pos=False)
    assert out.tobytes() == full[0].tobytes() and not pos.any()


def test_renderer_denoise_is_the_direct_call():
    """Renderer.denoise (scratch allocated once for any iteration count) returns what rt_denoise writes."""
    full = run_denoise(planes(), 3, abi.RT_DENOISE_DEMODULATE)
    dev = torch.device("cuda", 0)
    p = planes()
    h, w = p["prim_id"].shape
    r = Renderer(w, h)
    r.radiance = torch.from_numpy(np.array(p["color"])).to(dev).reshape(-1)
    r.normal_depth, r.albedo, r.prim_id = (torch.from_numpy(np.array(p[k])).to(dev)
                                           for k in ("normal_depth", "albedo", "prim_id"))
    img = r.denoise(3, *SIGMAS, demodulate=True, source="radiance")
    assert np.array_equal(img, full[1])
    assert r.denoised.cpu().numpy().tobytes() == full[0].tobytes()


def _e2e_renderer(ds, cfg):
    w, h = E2E_SIZE
    r = Renderer(w, h)
    r.render_init()
    r.render(ds, 1, cfg.depth, cfg.inputs(), radiance=True)
    return r


def test_end_to_end_lowers_the_error():
    """C5 scaled to 64x48, 1 spp, depth 4: render with radiance, gbuffer, denoise with the defaults.  Against the oracle's
    1024-spp radiance of the same frame the denoised float image has strictly lower mean squared error than the 1-spp
    input (the numpy reference filter satisfies this on the CPU: tests/test_denoise_host.py)."""
    e = end_to_end_frame()
    cfg = e["cfg"]
    ds = DeviceScene(e["scene"])
    r = _e2e_renderer(ds, cfg)
    r.gbuffer(ds, cfg.inputs())
    img = r.denoise()
    torch.cuda.synchronize()
    noisy, out = r.radiance_image(), r.denoised.cpu().numpy()
    before, after = mse(noisy, e["reference"]), mse(out, e["reference"])
    print(f"end to end: mse 1 spp {before:.5f}, denoised {after:.5f}")
    assert after < before
    assert np.array_equal(img, rgb_to_int_np(out[..., :3]))


def test_the_render_is_unchanged_by_the_passes():
    """rt_render's RGBA8 image and RNG states are the same whether or not gbuffer and denoise ran between frames."""
    e = end_to_end_frame()
    cfg = e["cfg"]
    ds = DeviceScene(e["scene"])
    plain = _e2e_renderer(ds, cfg)
    plain.render(ds, 1, cfg.depth, cfg.inputs(), radiance=True)
    torch.cuda.synchronize()
    mixed = _e2e_renderer(ds, cfg)
    mixed.gbuffer(ds, cfg.inputs())
    mixed.denoise()
    mixed.render(ds, 1, cfg.depth, cfg.inputs(), radiance=True)
    torch.cuda.synchronize()
    assert np.array_equal(plain.image(), mixed.image())
    assert np.array_equal(plain.states(), mixed.states())
    assert plain.radiance.cpu().numpy().tobytes() == mixed.radiance.cpu().numpy().tobytes()
