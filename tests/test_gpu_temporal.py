"""rt_temporal on the GPU against the numpy restatement of its definition (tests/test_temporal_host.py
temporal_reference).

Tolerance of the reference match: d = the largest absolute difference between the reference's own float32 and float64
runs on the case's decidable pixels (history and motion each have their own d).  The kernel may order a sum differently
or use another reciprocal or square root, each worth about one such spread, so 4·d is allowed: the denoiser test's factor,
for the same reason.  With the noise history d is 2e-4 .. 3e-3 (values of order 1-5; a wrong tap or weight errs by
0.1-1), at rest 2e-7.  "Has history" must agree exactly on decidable pixels.  The kernel performs the reference's float32
operations in the reference's order with IEEE division and square root, so its error is that of the float32 run: the
ratios are recorded in DESIGN.md §12."""
from __future__ import annotations

import ctypes as C

import numpy as np
import pytest
import torch

from cudaraytracer_amd import abi
from cudaraytracer_amd._lib import lib
from cudaraytracer_amd.renderer import DeviceScene, Renderer

from test_denoise_host import E2E_SIZE, UNDECIDABLE_CAP, end_to_end_frame, mixed_scene, mse, rgb_to_int_np, synthetic_planes
from test_temporal_host import (DEFAULTS, RESTING_CASES, SEQUENCE_FRAMES, TEMPORAL_CASES, _identity_inputs, numpy_sequence,
                                resting_expectation, sequence_inputs, sequence_reference, spread, temporal_case)

pytestmark = pytest.mark.gpu

PLANES = ("color", "normal_depth", "prim_id", "prev_history", "prev_normal_depth", "prev_prim_id")
FILL = -7.0


def run_temporal(case: dict, flags: int = 0, want_motion: bool = True, want_pos: bool = True, null_prev: bool = False,
                 expect: int = 0, **params) -> tuple:
    """(history (H, W, 4) float32, motion (H, W, 2) float32, pos (H, W) uint32) of one rt_temporal call on the case's
    planes (numpy, host); outputs the call does not write keep FILL / 0."""
    dev = torch.device("cuda", 0)
    h, w = case["prim_id"].shape
    t = {k: torch.from_numpy(np.array(case[k])).to(dev) for k in PLANES if not (null_prev and k.startswith("prev_"))}
    hist = torch.full((h, w, 4), FILL, dtype=torch.float32, device=dev)
    motion = torch.full((h, w, 2), FILL, dtype=torch.float32, device=dev)
    pos = torch.zeros((h, w), dtype=torch.int32, device=dev)
    a = abi.TemporalArgs()
    for k, v in t.items():
        setattr(a, k, v.data_ptr())
    a.history = hist.data_ptr()
    a.motion = motion.data_ptr() if want_motion else None
    a.pos = pos.data_ptr() if want_pos else None
    p = dict(DEFAULTS, **params)
    a.width, a.height, a.flags, a.max_history = w, h, flags, p["max_history"]
    a.depth_tol, a.normal_tol = p["depth_tol"], p["normal_tol"]
    a.tiling = abi.Tiling(h, 1, 0, h)
    a.inputs, a.prev_inputs = case["inputs"], case["prev_inputs"]
    rc = lib().rt_temporal(C.byref(a), C.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == expect, lib().rt_last_error()
    torch.cuda.synchronize()
    return hist.cpu().numpy(), motion.cpu().numpy(), pos.cpu().numpy().view(np.uint32)


@pytest.mark.parametrize("name", TEMPORAL_CASES)
def test_matches_the_reference(name):
    case = temporal_case(name)
    r64 = case["ref64"]
    m = r64["decidable"]
    assert 1.0 - float(m.mean()) <= UNDECIDABLE_CAP
    hist, motion, _ = run_temporal(case)
    for key, got in (("history", hist), ("motion", motion)):
        d = spread(case, key)
        err = float(np.abs(got.astype(np.float64) - r64[key])[m].max())
        print(f"{name} {key}: GPU error {err:.3e}, float32-vs-float64 spread d {d:.3e}, ratio {err / d if d else 0.0:.2f}")
        assert err <= 4 * d, (key, err, d)
    assert np.array_equal((hist[..., 3] > 1.0)[m], r64["has_history"][m])
    assert np.all(hist[..., 3] >= 1.0) and np.all(hist[..., 3] <= DEFAULTS["max_history"])
    assert np.all(motion[case["prim_id"] < 0] == 0)


@pytest.mark.parametrize("name", RESTING_CASES)
def test_resting_camera_is_bit_exact(name):
    """Identical cameras: every pixel reads its own history (one tap, weight 1); history = h + (1/N)·(c − h) as numpy
    float32 computes it, bit for bit; no motion."""
    case = temporal_case(name)
    hist, motion, _ = run_temporal(case)
    want, has = resting_expectation(case)
    assert hist.tobytes() == want.tobytes()
    assert not motion.any()
    assert np.array_equal(hist[..., 3] > 1.0, has)


def test_partial_tiles_and_a_narrow_frame():
    """A 9x5 crop of the synthetic planes (both halves, the miss band), resting camera: one partial workgroup."""
    full = temporal_case("rest_planes")
    case = {k: np.ascontiguousarray(full[k][10:15, 14:23]) for k in PLANES}
    case["inputs"] = case["prev_inputs"] = _identity_inputs()
    assert (case["prim_id"] < 0).any() and len(np.unique(case["prim_id"])) == 3
    hist, motion, pos = run_temporal(case)
    want, _ = resting_expectation(case)
    assert hist.shape == (5, 9, 4) and hist.tobytes() == want.tobytes()
    assert not motion.any()
    assert np.array_equal(pos, rgb_to_int_np(hist[..., :3]))


def test_reset_and_colour_as_a_sum():
    """RT_TEMPORAL_RESET, with the prev_* planes given or NULL: (colour, 1) everywhere.  RT_TEMPORAL_COLOR_IS_SUM:
    colour = rgb / w, 0 where w = 0 (synthetic_planes' accumulator), alone and blended into a resting history."""
    case = temporal_case("translate")
    for null_prev in (False, True):
        hist, motion, _ = run_temporal(case, abi.RT_TEMPORAL_RESET, null_prev=null_prev)
        assert hist[..., :3].tobytes() == case["color"][..., :3].tobytes()
        assert np.all(hist[..., 3] == 1.0) and not motion.any()
    rest = dict(temporal_case("rest_planes"))
    accum = synthetic_planes()["accum"]
    assert (accum[..., 3] == 0).any()
    w = accum[..., 3:4]
    mean = np.ones_like(accum)
    mean[..., :3] = np.where(w == 0, np.float32(0), accum[..., :3] / np.where(w == 0, np.float32(1), w))
    rest["color"] = accum
    flags = abi.RT_TEMPORAL_COLOR_IS_SUM
    hist, _, _ = run_temporal(rest, flags | abi.RT_TEMPORAL_RESET, null_prev=True)
    assert hist[..., :3].tobytes() == mean[..., :3].tobytes() and np.all(hist[..., 3] == 1.0)
    hist, _, _ = run_temporal(rest, flags)
    want, _ = resting_expectation(dict(rest, color=mean))
    assert hist.tobytes() == want.tobytes()


@pytest.mark.parametrize("name", ["large", "rest_planes"])
def test_pos_is_the_render_kernels_epilogue(name):
    """pos = rgb_to_int(255·sqrtf(history.rgb)) bit for bit (Kernel.cu:12-19, 152-157)."""
    hist, _, pos = run_temporal(temporal_case(name))
    assert np.array_equal(pos, rgb_to_int_np(hist[..., :3]))


def test_motion_and_pos_are_optional():
    case = temporal_case("rotate")
    full = run_temporal(case)
    hist, motion, pos = run_temporal(case, want_motion=False)
    assert hist.tobytes() == full[0].tobytes() and np.all(motion == FILL) and np.array_equal(pos, full[2])
    hist, motion, pos = run_temporal(case, want_pos=False)
    assert hist.tobytes() == full[0].tobytes() and motion.tobytes() == full[1].tobytes() and not pos.any()
    hist, motion, pos = run_temporal(case, want_motion=False, want_pos=False)
    assert hist.tobytes() == full[0].tobytes() and np.all(motion == FILL) and not pos.any()


def test_two_calls_give_the_same_bits():
    a, b = run_temporal(temporal_case("large")), run_temporal(temporal_case("large"))
    assert all(x.tobytes() == y.tobytes() for x, y in zip(a, b))


def test_aliasing_history_is_rejected_and_writes_nothing():
    dev = torch.device("cuda", 0)
    case = temporal_case("translate")
    h, w = case["prim_id"].shape
    t = {k: torch.from_numpy(np.array(case[k])).to(dev) for k in PLANES}
    a = abi.TemporalArgs()
    for k, v in t.items():
        setattr(a, k, v.data_ptr())
    a.history = t["prev_history"].data_ptr()
    a.width, a.height, a.max_history = w, h, 32
    a.depth_tol, a.normal_tol = 0.05, 0.2
    a.tiling = abi.Tiling(h, 1, 0, h)
    a.inputs, a.prev_inputs = case["inputs"], case["prev_inputs"]
    assert lib().rt_temporal(C.byref(a), None) == -1
    assert b"alias" in lib().rt_last_error()
    torch.cuda.synchronize()
    assert np.array_equal(t["prev_history"].cpu().numpy(), case["prev_history"])


def test_renderer_path_is_the_direct_call():
    """gbuffer(keep_previous=True) keeps the earlier planes and camera; Renderer.temporal (history planes ping-ponged,
    the first call a reset) returns what rt_temporal writes on the same planes."""
    case = temporal_case("translate")
    w, h = case["width"], case["height"]
    dev = torch.device("cuda", 0)
    ds = DeviceScene(mixed_scene())
    r = Renderer(w, h)
    first = r.gbuffer(ds, case["prev_inputs"], keep_previous=True)
    assert r.prev_normal_depth is None and r.prev_inputs is None
    nd0, id0 = first[0].cpu().numpy(), first[2].cpu().numpy()
    r.radiance = torch.from_numpy(np.array(case["prev_history"])).to(dev).reshape(-1)
    r.temporal()  # no previous G-buffer: a reset
    torch.cuda.synchronize()
    hist0 = r.history.cpu().numpy()
    assert hist0[..., :3].tobytes() == case["prev_history"][..., :3].tobytes() and np.all(hist0[..., 3] == 1.0)
    second = r.gbuffer(ds, case["inputs"], keep_previous=True)
    torch.cuda.synchronize()
    assert r.prev_normal_depth.cpu().numpy().tobytes() == nd0.tobytes()
    assert r.prev_prim_id.cpu().numpy().tobytes() == id0.tobytes()
    assert bytes(r.prev_inputs) == bytes(case["prev_inputs"])
    assert second[0].data_ptr() != r.prev_normal_depth.data_ptr()
    r.radiance = torch.from_numpy(np.array(case["color"])).to(dev).reshape(-1)
    pos = r.temporal(motion=True)
    torch.cuda.synchronize()
    direct = {"color": case["color"], "normal_depth": second[0].cpu().numpy(), "prim_id": second[2].cpu().numpy(),
              "prev_history": hist0, "prev_normal_depth": nd0, "prev_prim_id": id0, "inputs": case["inputs"],
              "prev_inputs": case["prev_inputs"]}
    hist, motion, want_pos = run_temporal(direct)
    assert r.history.cpu().numpy().tobytes() == hist.tobytes() and (hist[..., 3] > 1.0).any()
    assert r.motion.cpu().numpy().tobytes() == motion.tobytes()
    assert np.array_equal(pos.cpu().numpy().view(np.uint32).reshape(h, w), want_pos)
    # a third frame swaps back: the second frame's planes are the previous ones, its history is read
    nd1 = second[0].cpu().numpy()
    r.gbuffer(ds, case["prev_inputs"], keep_previous=True)
    r.temporal()
    torch.cuda.synchronize()
    assert r.prev_normal_depth.cpu().numpy().tobytes() == nd1.tobytes()
    assert bytes(r.prev_inputs) == bytes(case["inputs"])
    assert (r.history.cpu().numpy()[..., 3] > 2.0).any()
    # the default call leaves one plane set in place
    keep = r.normal_depth.data_ptr()
    r.gbuffer(ds, case["inputs"])
    assert r.normal_depth.data_ptr() == keep


def _sequence(ds, cfg, passes: bool):
    """Six frames of the orbit through render (→ gbuffer → temporal); returns the renderer and, with the passes, each
    frame's radiance and G-buffer planes (host copies)."""
    w, h = E2E_SIZE
    r = Renderer(w, h)
    r.render_init()
    frames, gbuffers = [], []
    for k in range(SEQUENCE_FRAMES):
        inp = sequence_inputs(k)
        r.render(ds, 1, cfg.depth, inp, radiance=True)
        if passes:
            nd, alb, ids = r.gbuffer(ds, inp, keep_previous=True)
            r.temporal()
            torch.cuda.synchronize()
            frames.append(r.radiance_image().copy())
            gbuffers.append({"normal_depth": nd.cpu().numpy(), "albedo": alb.cpu().numpy(), "prim_id": ids.cpu().numpy()})
    torch.cuda.synchronize()
    return r, frames, gbuffers


def test_end_to_end_sequence_lowers_the_error():
    """C5 at 64x48, 1 spp, depth 4, six frames at 1 degree per frame through render → gbuffer → temporal → denoise.
    Against the oracle's 1024-spp radiance of the last frame, the result's mean squared error is within 10 % of the
    numpy pipeline's on the same rendered frames and G-buffers (the two differ only at undecidable pixels) and strictly
    below that of denoise alone on the last frame."""
    e = end_to_end_frame()
    ds = DeviceScene(e["scene"])
    r, frames, gbuffers = _sequence(ds, e["cfg"], True)
    r.denoise(source="history")
    torch.cuda.synchronize()
    both = r.denoised.cpu().numpy().copy()
    r.denoise(source="radiance")
    torch.cuda.synchronize()
    alone = r.denoised.cpu().numpy()
    ref = sequence_reference()
    want = numpy_sequence(frames, gbuffers)
    got, expected, filt, raw = mse(both, ref), mse(want["temporal_filtered"], ref), mse(alone, ref), mse(frames[-1], ref)
    temp = mse(r.history.cpu().numpy(), ref)
    print(f"sequence: mse raw {raw:.5f}, denoise alone {filt:.5f}, temporal alone {temp:.5f}, temporal then denoise "
          f"{got:.5f} (numpy pipeline {expected:.5f})")
    assert abs(got - expected) <= 0.1 * expected
    assert got < filt
    assert (r.history.cpu().numpy()[..., 3] >= SEQUENCE_FRAMES - 0.5).any()


def test_the_render_is_unchanged_by_the_pass():
    """rt_render's image, radiance and RNG states are the same whether or not gbuffer and temporal ran between frames."""
    e = end_to_end_frame()
    ds = DeviceScene(e["scene"])
    plain, _, _ = _sequence(ds, e["cfg"], False)
    mixed, _, _ = _sequence(ds, e["cfg"], True)
    assert np.array_equal(plain.image(), mixed.image())
    assert np.array_equal(plain.states(), mixed.states())
    assert plain.radiance.cpu().numpy().tobytes() == mixed.radiance.cpu().numpy().tobytes()
