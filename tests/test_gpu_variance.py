"""rt_temporal_moments and rt_denoise_variance on the GPU against the numpy restatements of their definitions
(tests/test_variance_host.py moments_reference, variance_filter_reference) and against rt_temporal / rt_temporal_dynamic.

Tolerances, by the rule of test_gpu_temporal.py and test_gpu_denoise.py: d = the largest absolute difference between the
reference's own float32 and float64 runs (moments: on the case's decidable pixels; filter: colour and variance each
have their own d); the kernel may order a sum differently, contract a multiply-add or use another exponential, each worth
about one such spread, so 4·d is allowed.  Every test prints its d.  Measured on MI355X: moments d = 5·10⁻⁷ (at rest) ..
1.3·10⁻⁴, GPU error / d = 1.00 on all five cases; filter d = 2.8·10⁻⁷ .. 1.4·10⁻⁶ (rgb) and 1.2·10⁻⁸ .. 7.5·10⁻⁸
(variance), error / d between 0.97 and 1.69."""
from __future__ import annotations

import ctypes as C
import functools

import numpy as np
import pytest
import torch

from cudaraytracer_amd import abi
from cudaraytracer_amd._lib import lib
from cudaraytracer_amd.renderer import DeviceScene, Renderer

from test_denoise_host import E2E_SIZE, UNDECIDABLE_CAP, end_to_end_frame, mixed_scene, mse, rgb_to_int_np
from test_dynamic_host import CROP_SIZE, crop_case, dynamic_case
from test_temporal_host import (DEFAULTS, RESTING_CASES, SEQUENCE_FRAMES, _identity_inputs, sequence_inputs,
                                sequence_reference, temporal_case)
from test_variance_host import (VARIANCE_DEFAULTS, moments_reference, numpy_variance_sequence, reset_moments,
                                variance_filter_reference, variance_planes)

pytestmark = pytest.mark.gpu

F = np.float32
PLANES = ("color", "normal_depth", "prim_id", "prev_history", "prev_normal_depth", "prev_prim_id")
FILL = -7.0
GUARD = 3  # rows of the output tensors before and after the frame that no call may write


def case_with_moments(case: dict, seed: int) -> dict:
    """The temporal case plus a seeded previous moments plane (gamma noise) and, if it has none, no motion table."""
    h, w = case["prim_id"].shape
    out = dict(case)
    out["prev_moments"] = np.random.default_rng(seed).gamma(2.0, 0.5, (h, w, 2)).astype(F)
    out.setdefault("prim_motion", None)
    return out


@functools.lru_cache(maxsize=None)
def moments_case(name: str) -> dict:
    """A case of the moments pass with its float64 / float32 references; computed once per process, read-only."""
    if name == "crop":
        case = case_with_moments(crop_case(), 71)
    elif name == "object_and_camera":
        case = case_with_moments(dynamic_case(name), 72)
    else:
        case = case_with_moments(temporal_case(name), 73 + len(name))
    args = tuple(case[k] for k in PLANES) + (case["prev_moments"], case["inputs"], case["prev_inputs"], case["prim_motion"])
    case["mref64"] = moments_reference(*args, **DEFAULTS, dtype=np.float64)
    case["mref32"] = moments_reference(*args, **DEFAULTS, dtype=np.float32)
    return case


def run_moments(case: dict, flags: int = 0, null_prev: bool = False, with_moments: bool = True, guard: int = 0) -> dict:
    """history, motion, pos and (with_moments) moments of one call on the case's planes (numpy, host): rt_temporal_moments,
    or without moments rt_temporal / rt_temporal_dynamic, by whether the case has a motion table.  guard > 0: the
    outputs live in the middle rows of taller tensors filled with FILL / 0, and those rows are returned too."""
    dev = torch.device("cuda", 0)
    h, w = case["prim_id"].shape
    t = {k: torch.from_numpy(np.array(case[k])).to(dev) for k in PLANES if not (null_prev and k.startswith("prev_"))}
    rows = h + 2 * guard
    hist = torch.full((rows, w, 4), FILL, dtype=torch.float32, device=dev)
    motion = torch.full((rows, w, 2), FILL, dtype=torch.float32, device=dev)
    mom = torch.full((rows, w, 2), FILL, dtype=torch.float32, device=dev)
    pos = torch.zeros((rows, w), dtype=torch.int32, device=dev)
    prev_m = None if null_prev else torch.from_numpy(np.array(case["prev_moments"])).to(dev)
    a = abi.TemporalArgs()
    for k, v in t.items():
        setattr(a, k, v.data_ptr())
    a.history, a.motion, a.pos = hist[guard:].data_ptr(), motion[guard:].data_ptr(), pos[guard:].data_ptr()
    a.width, a.height, a.flags, a.max_history = w, h, flags, DEFAULTS["max_history"]
    a.depth_tol, a.normal_tol = DEFAULTS["depth_tol"], DEFAULTS["normal_tol"]
    a.tiling = abi.Tiling(h, 1, 0, h)
    a.inputs = case["inputs"]
    a.prev_inputs = case["prev_inputs"] if case["prev_inputs"] is not None else case["inputs"]
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    table = case.get("prim_motion")
    dtable = None if table is None else torch.from_numpy(np.array(table, dtype=F)).to(dev)
    tp, tn = (None, 0) if dtable is None else (C.c_void_p(dtable.data_ptr()), dtable.shape[0])
    if with_moments:
        rc = lib().rt_temporal_moments(C.byref(a), tp, tn, None if prev_m is None else C.c_void_p(prev_m.data_ptr()),
                                       C.c_void_p(mom[guard:].data_ptr()), stream)
    elif dtable is None:
        rc = lib().rt_temporal(C.byref(a), stream)
    else:
        rc = lib().rt_temporal_dynamic(C.byref(a), tp, tn, stream)
    assert rc == 0, lib().rt_last_error()
    torch.cuda.synchronize()
    return {"history": hist.cpu().numpy(), "motion": motion.cpu().numpy(), "pos": pos.cpu().numpy().view(np.uint32),
            "moments": mom.cpu().numpy()}


def check_moments(case: dict, got: np.ndarray, label: str) -> None:
    r64, r32 = case["mref64"], case["mref32"]
    m = r64["decidable"]
    share = 1.0 - float(m.mean())
    assert share <= UNDECIDABLE_CAP
    d = float(np.abs(r32["moments"].astype(np.float64) - r64["moments"])[m].max())
    err = float(np.abs(got.astype(np.float64) - r64["moments"])[m].max())
    print(f"{label} moments: GPU error {err:.3e}, float32-vs-float64 spread d {d:.3e}, ratio {err / d if d else 0.0:.2f}, "
          f"undecidable {share:.4f}")
    assert err <= 4 * d, (err, d)


@pytest.mark.parametrize("name", ["translate", "c2", "rest_mixed", "object_and_camera"])
def test_moments_pass_matches_the_reference_and_the_plain_pass(name):
    """50x37 (translate, rest_mixed, object_and_camera: the last through the motion table) and 64x40 (c2)."""
    case = moments_case(name)
    assert (case["prim_id"].shape[::-1]) in ((50, 37), (64, 40))
    got, plain = run_moments(case), run_moments(case, with_moments=False)
    for key in ("history", "motion", "pos"):
        assert got[key].tobytes() == plain[key].tobytes(), key
    assert np.all(plain["moments"] == FILL) and (got["history"][..., 3] > 1.0).any()
    check_moments(case, got["moments"], name)


def resting_moments(case: dict) -> np.ndarray:
    """(H, W, 2) float32 of a resting camera, written out directly: m + (1/N)·((l, l·l) − m), or (l, l·l) without history."""
    h = case["prev_history"]
    has = (case["prim_id"] >= 0) & (case["prev_prim_id"] == case["prim_id"]) & (h[..., 3] > 0)
    alpha = (F(1) / np.minimum(h[..., 3] + F(1), F(DEFAULTS["max_history"])).astype(F)).astype(F)[..., None]
    fresh, m = reset_moments(case["color"]), case["prev_moments"]
    return np.where(has[..., None], m + alpha * (fresh - m), fresh).astype(F)


@pytest.mark.parametrize("name", RESTING_CASES)
def test_resting_camera_moments_are_the_running_mean_bit_for_bit(name):
    case = case_with_moments(temporal_case(name), 5)
    got = run_moments(case)
    assert got["moments"].tobytes() == resting_moments(case).tobytes()
    assert got["history"].tobytes() == run_moments(case, with_moments=False)["history"].tobytes()


def test_reset_gives_the_luminance_and_its_square():
    case = case_with_moments(temporal_case("translate"), 6)
    want = reset_moments(case["color"])
    for null_prev in (False, True):
        got = run_moments(case, abi.RT_TEMPORAL_RESET, null_prev=null_prev)
        assert got["moments"].tobytes() == want.tobytes()
        assert got["history"][..., :3].tobytes() == case["color"][..., :3].tobytes() and np.all(got["history"][..., 3] == 1.0)
    case = case_with_moments(temporal_case("c2"), 7)  # (the scene with sky: a miss gets (l, l·l) too)
    miss = case["prim_id"] < 0
    got = run_moments(case)
    assert miss.any() and got["moments"][miss].tobytes() == reset_moments(case["color"])[miss].tobytes()


def assert_guard_rows_untouched(got: dict, h: int) -> None:
    for key, fill in (("history", FILL), ("motion", FILL), ("moments", FILL), ("pos", 0)):
        plane = got[key]
        assert plane.shape[0] == h + 2 * GUARD
        assert np.all(plane[:GUARD] == fill) and np.all(plane[GUARD + h:] == fill), key


def test_partial_tiles_write_nothing_outside_the_frame():
    """70x9 through the motion table: two workgroups across, the second 6 pixels wide; three down, the last one row high."""
    case = moments_case("crop")
    w, h = CROP_SIZE
    got = run_moments(case, guard=GUARD)
    assert_guard_rows_untouched(got, h)
    inner = {k: v[GUARD:GUARD + h] for k, v in got.items()}
    plain = run_moments(case, with_moments=False)
    for key in ("history", "motion", "pos"):
        assert inner[key].tobytes() == plain[key].tobytes(), key
    check_moments(case, inner["moments"], "70x9")


def test_a_narrow_crop_at_rest():
    """A 9x5 crop of the synthetic planes (both halves, the miss band), resting camera: one partial workgroup."""
    full = temporal_case("rest_planes")
    case = {k: np.ascontiguousarray(full[k][10:15, 14:23]) for k in PLANES}
    case["inputs"] = case["prev_inputs"] = _identity_inputs()
    case = case_with_moments(case, 8)
    assert (case["prim_id"] < 0).any() and len(np.unique(case["prim_id"])) == 3
    got = run_moments(case, guard=GUARD)
    assert_guard_rows_untouched(got, 5)
    assert got["moments"][GUARD:GUARD + 5].tobytes() == resting_moments(case).tobytes()


# ---------------------------------------------------------------------------------------------------------------------
# The filter
# ---------------------------------------------------------------------------------------------------------------------
def run_variance(planes: dict, iterations: int, want_pos: bool = True, want_out: bool = True, **params) -> tuple:
    """(out_color (H, W, 4) float32, pos (H, W) uint32) of one rt_denoise_variance call on the planes (numpy, host)."""
    dev = torch.device("cuda", 0)
    h, w = planes["prim_id"].shape
    t = {k: torch.from_numpy(np.array(planes[k])).to(dev) for k in ("color", "moments", "normal_depth", "prim_id")}
    out = torch.full((h, w, 4), FILL, dtype=torch.float32, device=dev)
    pos = torch.zeros((h, w), dtype=torch.int32, device=dev)
    scratch = torch.zeros(int(lib().rt_denoise_variance_scratch_bytes(w, h, iterations)), dtype=torch.uint8, device=dev)
    p = dict(VARIANCE_DEFAULTS, **params)
    a = abi.DenoiseVarianceArgs()
    for k, v in t.items():
        setattr(a, k, v.data_ptr())
    a.out_color = out.data_ptr() if want_out else None
    a.pos = pos.data_ptr() if want_pos else None
    a.scratch = scratch.data_ptr()
    a.width, a.height, a.iterations, a.min_history = w, h, iterations, p["min_history"]
    a.sigma_l, a.sigma_n, a.sigma_z = p["sigma_l"], p["sigma_n"], p["sigma_z"]
    a.tiling = abi.Tiling(h, 1, 0, h)
    rc = lib().rt_denoise_variance(C.byref(a), C.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0, lib().rt_last_error()
    torch.cuda.synchronize()
    return out.cpu().numpy(), pos.cpu().numpy().view(np.uint32)


@functools.lru_cache(maxsize=None)
def filter_case(width: int, height: int, iterations: int) -> tuple:
    p = variance_planes(width, height)
    args = (p["color"], p["moments"], p["normal_depth"], p["prim_id"])
    kw = dict(VARIANCE_DEFAULTS, iterations=iterations)
    return p, variance_filter_reference(*args, **kw, dtype=np.float64), variance_filter_reference(*args, **kw, dtype=np.float32)


def check_filter(width: int, height: int, iterations: int) -> None:
    p, r64, r32 = filter_case(width, height, iterations)
    n = p["color"][..., 3]
    assert n.min() == 1 and n.max() == 8 and (n < 4).any() and (n >= 4).any()
    out, pos = run_variance(p, iterations)
    for label, sl in (("rgb", np.s_[..., :3]), ("variance", np.s_[..., 3])):
        d = float(np.abs(r32[sl].astype(np.float64) - r64[sl]).max())
        err = float(np.abs(out[sl].astype(np.float64) - r64[sl]).max())
        print(f"{width}x{height} N={iterations} {label}: GPU error {err:.3e}, float32-vs-float64 spread d {d:.3e}, "
              f"ratio {err / d:.2f}")
        assert d > 0
        assert err <= 4 * d, (label, err, d)
    assert np.array_equal(pos, rgb_to_int_np(out[..., :3]))
    miss = p["prim_id"] < 0
    assert miss.any() and out[..., :3][miss].tobytes() == p["color"][..., :3][miss].tobytes()
    assert not out[..., 3][miss].any() and np.all(out[..., 3] >= 0)
    again = run_variance(p, iterations)
    assert again[0].tobytes() == out.tobytes() and again[1].tobytes() == pos.tobytes()


@pytest.mark.parametrize("iterations", [1, 3, 5])
def test_filter_matches_the_reference(iterations):
    """37x29: history lengths on both sides of min_history, a zero-variance patch, the miss band; N = 5 reaches the
    global-memory build, whose taps leave the frame on every side."""
    check_filter(37, 29, iterations)


def test_filter_on_partial_tiles_with_the_global_memory_build():
    """70x41 (three workgroups across and down, the last ones partial), N = 4: steps 1, 2, 4 from LDS and 8 from memory."""
    check_filter(70, 41, 4)


def test_each_output_is_optional():
    p, _, _ = filter_case(37, 29, 3)
    full = run_variance(p, 3)
    out, pos = run_variance(p, 3, want_out=False)
    assert np.array_equal(pos, full[1]) and np.all(out == FILL)
    out, pos = run_variance(p, 3, want_pos=False)
    assert out.tobytes() == full[0].tobytes() and not pos.any()


# ---------------------------------------------------------------------------------------------------------------------
# Aliasing, the Python layer, end to end
# ---------------------------------------------------------------------------------------------------------------------
def test_aliasing_calls_are_rejected_and_write_nothing():
    dev = torch.device("cuda", 0)
    case = case_with_moments(temporal_case("translate"), 9)
    h, w = case["prim_id"].shape
    t = {k: torch.from_numpy(np.array(case[k])).to(dev) for k in PLANES + ("prev_moments",)}
    hist = torch.full((h, w, 4), FILL, dtype=torch.float32, device=dev)
    a = abi.TemporalArgs()
    for k in PLANES:
        setattr(a, k, t[k].data_ptr())
    a.history = hist.data_ptr()
    a.width, a.height, a.max_history = w, h, 32
    a.depth_tol, a.normal_tol = 0.05, 0.2
    a.tiling = abi.Tiling(h, 1, 0, h)
    a.inputs, a.prev_inputs = case["inputs"], case["prev_inputs"]
    pm = C.c_void_p(t["prev_moments"].data_ptr())
    assert lib().rt_temporal_moments(C.byref(a), None, 0, pm, pm, None) == -1
    assert b"moments" in lib().rt_last_error()
    torch.cuda.synchronize()
    assert np.array_equal(t["prev_moments"].cpu().numpy(), case["prev_moments"]) and np.all(hist.cpu().numpy() == FILL)
    # the filter: out_color over the colour plane
    p, _, _ = filter_case(37, 29, 3)
    h, w = p["prim_id"].shape
    f = {k: torch.from_numpy(np.array(p[k])).to(dev) for k in ("color", "moments", "normal_depth", "prim_id")}
    scratch = torch.zeros(int(lib().rt_denoise_variance_scratch_bytes(w, h, 3)), dtype=torch.uint8, device=dev)
    v = abi.DenoiseVarianceArgs()
    for k, x in f.items():
        setattr(v, k, x.data_ptr())
    v.out_color, v.scratch = f["color"].data_ptr(), scratch.data_ptr()
    v.width, v.height, v.iterations, v.min_history = w, h, 3, 4
    v.sigma_l, v.sigma_n, v.sigma_z = 1.0, 0.1, 0.05
    v.tiling = abi.Tiling(h, 1, 0, h)
    assert lib().rt_denoise_variance(C.byref(v), None) == -1
    assert b"alias" in lib().rt_last_error()
    torch.cuda.synchronize()
    assert np.array_equal(f["color"].cpu().numpy(), p["color"]) and not scratch.any().item()


def test_renderer_path_is_the_direct_calls():
    """Renderer.temporal(moments=True) (moments planes ping-ponged beside the history, the first call a reset) and
    Renderer.denoise_variance() return what the two entry points write on the same planes."""
    case = temporal_case("translate")
    w, h = case["width"], case["height"]
    dev = torch.device("cuda", 0)
    ds = DeviceScene(mixed_scene())
    r = Renderer(w, h)
    first = r.gbuffer(ds, case["prev_inputs"], keep_previous=True)
    nd0, id0 = first[0].cpu().numpy(), first[2].cpu().numpy()
    r.radiance = torch.from_numpy(np.array(case["prev_history"])).to(dev).reshape(-1)
    r.temporal(moments=True)  # no previous G-buffer: a reset
    torch.cuda.synchronize()
    hist0, mom0 = r.history.cpu().numpy(), r.moments.cpu().numpy()
    assert mom0.tobytes() == reset_moments(case["prev_history"]).tobytes() and np.all(hist0[..., 3] == 1.0)
    second = r.gbuffer(ds, case["inputs"], keep_previous=True)
    r.radiance = torch.from_numpy(np.array(case["color"])).to(dev).reshape(-1)
    pos = r.temporal(motion=True, moments=True)
    torch.cuda.synchronize()
    direct = {"color": case["color"], "normal_depth": second[0].cpu().numpy(), "prim_id": second[2].cpu().numpy(),
              "prev_history": hist0, "prev_normal_depth": nd0, "prev_prim_id": id0, "prev_moments": mom0,
              "inputs": case["inputs"], "prev_inputs": case["prev_inputs"], "prim_motion": None}
    want = run_moments(direct)
    assert r.history.cpu().numpy().tobytes() == want["history"].tobytes() and (want["history"][..., 3] > 1.0).any()
    assert r.moments.cpu().numpy().tobytes() == want["moments"].tobytes()
    assert r.motion.cpu().numpy().tobytes() == want["motion"].tobytes()
    assert np.array_equal(pos.cpu().numpy().view(np.uint32).reshape(h, w), want["pos"])
    assert r.moments.data_ptr() != r._moments_spare.data_ptr()
    img = r.denoise_variance()
    planes = {"color": want["history"], "moments": want["moments"], "normal_depth": direct["normal_depth"],
              "prim_id": direct["prim_id"]}
    out, want_img = run_variance(planes, 3)
    assert r.denoised_variance.cpu().numpy().tobytes() == out.tobytes() and np.array_equal(img, want_img)
    # with a motion table the same call goes through the dynamic body: the identity table gives the same bits
    table = np.zeros((int(direct["prim_id"].max()) + 1, 4), dtype=F)
    table[:, 3] = 1.0
    assert run_moments(dict(direct, prim_motion=table))["moments"].tobytes() == want["moments"].tobytes()


def _sequence(ds, cfg, passes: bool):
    """Six frames of the orbit through render (→ gbuffer → temporal with moments); returns the renderer and, with the
    passes, each frame's radiance and G-buffer planes (host copies)."""
    w, h = E2E_SIZE
    r = Renderer(w, h)
    r.render_init()
    frames, gbuffers = [], []
    for k in range(SEQUENCE_FRAMES):
        inp = sequence_inputs(k)
        r.render(ds, 1, cfg.depth, inp, radiance=True)
        if passes:
            nd, alb, ids = r.gbuffer(ds, inp, keep_previous=True)
            r.temporal(moments=True)
            r.denoise_variance_async()
            torch.cuda.synchronize()
            frames.append(r.radiance_image().copy())
            gbuffers.append({"normal_depth": nd.cpu().numpy(), "albedo": alb.cpu().numpy(), "prim_id": ids.cpu().numpy()})
    torch.cuda.synchronize()
    return r, frames, gbuffers


def test_end_to_end_sequence_matches_the_numpy_pipeline():
    """C5 at 64x48, 1 spp, depth 4, six frames at 1 degree per frame through render → gbuffer → temporal with moments →
    denoise_variance, and the last frame alone through a reset and the filter.  Against the oracle's 1024-spp radiance of
    the last frame, both results' mean squared errors are within 10 % of the numpy pipeline's on the same rendered frames
    and G-buffers (the margin of test_gpu_temporal.py: the two differ only at undecidable pixels)."""
    e = end_to_end_frame()
    ds = DeviceScene(e["scene"])
    r, frames, gbuffers = _sequence(ds, e["cfg"], True)
    r.denoise_variance()
    torch.cuda.synchronize()
    both = r.denoised_variance.cpu().numpy().copy()
    temp = r.history.cpu().numpy().copy()
    r.temporal(moments=True, reset=True)  # the last frame as a history of length 1
    r.denoise_variance()
    torch.cuda.synchronize()
    alone = r.denoised_variance.cpu().numpy()
    ref = sequence_reference()
    want = numpy_variance_sequence(frames, gbuffers)
    got_a, want_a = mse(both, ref), mse(want["temporal_filtered"], ref)
    got_b, want_b = mse(alone, ref), mse(want["filtered"], ref)
    print(f"sequence: temporal alone {mse(temp, ref):.5f}; history filtered {got_a:.5f} (numpy pipeline {want_a:.5f}); "
          f"raw frame filtered {got_b:.5f} (numpy pipeline {want_b:.5f})")
    assert abs(got_a - want_a) <= 0.1 * want_a
    assert abs(got_b - want_b) <= 0.1 * want_b
    assert (temp[..., 3] >= SEQUENCE_FRAMES - 0.5).any()


def test_the_render_is_unchanged_by_the_passes():
    """rt_render's image, radiance and RNG states are the same whether or not gbuffer, temporal with moments and the
    variance-guided filter ran between frames."""
    e = end_to_end_frame()
    ds = DeviceScene(e["scene"])
    plain, _, _ = _sequence(ds, e["cfg"], False)
    mixed, _, _ = _sequence(ds, e["cfg"], True)
    mixed.denoise_variance()
    torch.cuda.synchronize()
    assert np.array_equal(plain.image(), mixed.image())
    assert np.array_equal(plain.states(), mixed.states())
    assert plain.radiance.cpu().numpy().tobytes() == mixed.radiance.cpu().numpy().tobytes()
