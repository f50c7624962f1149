"""rt_temporal without a device: the entry point's argument checks, the struct layout, and temporal_reference, the
numpy restatement of the definition in include/rt_hip.h that the GPU tests (test_gpu_temporal.py) import.

temporal_reference evaluates the definition in float64 or in float32 (every operation in that type, in the order the
kernel performs them) and returns the history plane, the motion plane, "has history" and, from the float64 run, a
`decidable` mask.  A pixel is undecidable when any threshold the definition tests lies within a relative 1e-3 of its
limit for a tap that passes the other tests: s and den against 0 (margins 1e-3 and 1e-3·(|near'| + |far'|): their limit
is 0, so the margin is relative to the quantities' own scale), the snap distance against 1/256, the depth difference
against depth_tol·max(t_exp, 1e-3), the normals' dot product against 1 − normal_tol, and S against 1/100.  There a
float32 evaluation may legitimately decide the other way.  At most 3 % of a case's pixels may be undecidable: asserted
here on the reference alone, and again by the GPU tests.

The geometry cases take both G-buffers from gbuffer_reference (test_denoise_host.py); history rgb and colour are gamma
noise, history lengths random integers 0..39 (zero-length taps and the max_history cap both occur)."""
from __future__ import annotations

import ctypes as C
import functools
import math

import numpy as np
import pytest

from cudaraytracer_amd import abi, scenes
from cudaraytracer_amd._lib import EXPORTED, lib
from oracle import py_oracle as po

from test_denoise_host import (E2E_SIZE, UNDECIDABLE_CAP, camera_rays, end_to_end_frame, filter_reference, gbuffer_case,
                               gbuffer_reference, mixed_scene, mse, synthetic_planes)

F = np.float32
MARGIN = 1e-3
SNAP = 1.0 / 256.0
MIN_WEIGHT = 1.0 / 100.0
DEFAULTS = {"max_history": 32, "depth_tol": 0.05, "normal_tol": 0.2}


# ---------------------------------------------------------------------------------------------------------------------
# The definition in numpy
# ---------------------------------------------------------------------------------------------------------------------
def _dot(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def _camera(inputs: abi.InputStruct, f) -> dict:
    """The launch-uniform camera terms of Kernel.cu:130-143 in type f."""
    up, fw, origin = (np.array([v[0], v[1], v[2]], dtype=f) for v in (inputs.up, inputs.orientation, inputs.origin))
    cr = np.array([up[1] * fw[2] - up[2] * fw[1], -(up[0] * fw[2] - up[2] * fw[0]), up[0] * fw[1] - up[1] * fw[0]], dtype=f)
    right = (f(1) / np.sqrt((cr[0] * cr[0] + cr[1] * cr[1]) + cr[2] * cr[2])) * cr
    fov = f(inputs.fov)
    k10 = (f(1) / fov) * f(10)
    return {"origin": origin, "fw": fw, "up": up, "right": right.astype(f), "fov": fov, "k10": k10,
            "near": f(inputs.near_plane), "far": f(inputs.far_plane), "fov_fwd": fov * fw, "k10_fwd": k10 * fw,
            "ff": (fw[0] * fw[0] + fw[1] * fw[1]) + fw[2] * fw[2]}


def _ray_start(cam: dict, u, v):
    dist = u[..., None] * cam["right"] + v[..., None] * cam["up"]
    return (cam["near"] * dist + cam["origin"]) + cam["fov_fwd"], dist


def temporal_reference(color, normal_depth, prim_id, prev_history, prev_normal_depth, prev_prim_id, inputs, prev_inputs,
                       max_history=32, depth_tol=0.05, normal_tol=0.2, flags=0, dtype=np.float64) -> dict:
    """history (H, W, 4), motion (H, W, 2) of `dtype`, has_history (H, W) and decidable (H, W) of rt_temporal.  The
    planes are the float32 / int32 arrays the kernel reads; the tolerances are rounded to float32 first, as
    rt_temporal_args holds them, and 1 − normal_tol is formed in float32, as the library does."""
    f = dtype
    prim = np.asarray(prim_id)
    hgt, wid = prim.shape
    col = np.asarray(color).astype(f)
    if flags & abi.RT_TEMPORAL_COLOR_IS_SUM:
        w = col[..., 3:4]
        with np.errstate(divide="ignore", invalid="ignore"):
            c = np.where(w == 0, f(0), col[..., :3] / np.where(w == 0, f(1), w)).astype(f)
    else:
        c = col[..., :3].copy()
    history = np.concatenate([c, np.ones((hgt, wid, 1), dtype=f)], axis=-1)
    motion = np.zeros((hgt, wid, 2), dtype=f)
    has = np.zeros((hgt, wid), dtype=bool)
    decidable = np.ones((hgt, wid), dtype=bool)
    if flags & abi.RT_TEMPORAL_RESET:
        return {"history": history, "motion": motion, "has_history": has, "decidable": decidable}
    hit = prim >= 0
    nd = np.asarray(normal_depth).astype(f)
    ph, pnd, pprim = np.asarray(prev_history).astype(f), np.asarray(prev_normal_depth).astype(f), np.asarray(prev_prim_id)
    cur, prv = _camera(inputs, f), _camera(prev_inputs, f)
    W, half_w, half_h = f(wid), f(wid) / f(2), f(hgt) / f(2)
    ys, xs = np.mgrid[0:hgt, 0:wid]
    xf, yf = xs.astype(f), ys.astype(f)
    with np.errstate(all="ignore"):
        # 1. the world point on the centre ray
        u = ((xf - half_w) + f(0.5)) / W
        v = ((half_h - yf) + f(0.5)) / W
        ro, dist = _ray_start(cur, u, v)
        second = (cur["far"] * dist + cur["k10_fwd"]) + cur["origin"]
        d = second - ro
        rd = (f(1) / np.sqrt(_dot(d, d)))[..., None] * d
        P = ro + nd[..., 3:4] * rd
        # 2. the inverse of the ray construction under the previous camera
        q = P - prv["origin"]
        a, b = _dot(q, prv["right"][None, None]), _dot(q, prv["up"][None, None])
        cf = _dot(q, prv["fw"][None, None]) / prv["ff"]
        s = (cf - prv["fov"]) / (prv["k10"] - prv["fov"])
        den = prv["near"] + s * (prv["far"] - prv["near"])
        ok2 = hit & (s > 0) & (den > 0)
        up_, vp = a / den, b / den
        px = (up_ * W + half_w) - f(0.5)
        py = (half_h + f(0.5)) - vp * W
        e = P - _ray_start(prv, up_, vp)[0]
        t_exp = np.sqrt(_dot(e, e))
        # 3. snap
        dx, dy = np.abs(px - np.rint(px)), np.abs(py - np.rint(py))
        px = np.where(dx <= f(SNAP), np.rint(px), px).astype(f)
        py = np.where(dy <= f(SNAP), np.rint(py), py).astype(f)
        motion[ok2, 0] = (px - xf)[ok2]
        motion[ok2, 1] = (py - yf)[ok2]
        # 4. bilinear fetch
        inr = ok2 & (px > -1) & (px < W) & (py > -1) & (py < f(hgt))
        pxc, pyc = np.where(inr, px, f(0)), np.where(inr, py, f(0))
        x0f, y0f = np.floor(pxc), np.floor(pyc)
        fx, fy = pxc - x0f, pyc - y0f
        x0, y0 = x0f.astype(np.int64), y0f.astype(np.int64)
        wx, wy = (f(1) - fx, fx), (f(1) - fy, fy)
        lim = f(F(depth_tol)) * np.maximum(t_exp, f(F(1e-3)))
        min_ndot = f(F(1.0) - F(normal_tol))
        S = np.zeros((hgt, wid), dtype=f)
        acc = np.zeros((hgt, wid, 4), dtype=f)
        near = np.zeros((hgt, wid), dtype=bool)  # a tap's depth or normal test within the margin
        for k in range(4):
            i, j = k & 1, k >> 1
            wk = wx[i] * wy[j]
            xi, yj = x0 + i, y0 + j
            base = inr & (wk > 0) & (xi >= 0) & (xi < wid) & (yj >= 0) & (yj < hgt)
            xi, yj = np.clip(xi, 0, wid - 1), np.clip(yj, 0, hgt - 1)
            hq, nq = ph[yj, xi], pnd[yj, xi]
            base = base & (pprim[yj, xi] == prim) & (hq[..., 3] > 0)
            dz = np.abs(nq[..., 3] - t_exp)
            ndot = (nd[..., 0] * nq[..., 0] + nd[..., 1] * nq[..., 1]) + nd[..., 2] * nq[..., 2]
            pass_z, pass_n = dz <= lim, ndot >= min_ndot
            near_z, near_n = np.abs(dz - lim) <= MARGIN * lim, np.abs(ndot - min_ndot) <= MARGIN * abs(min_ndot)
            near |= base & ((near_z & (pass_n | near_n)) | (near_n & (pass_z | near_z)))
            wk = np.where(base & pass_z & pass_n, wk, f(0)).astype(f)
            S = S + wk
            acc = acc + wk[..., None] * hq
        has = inr & (S >= f(MIN_WEIGHT))
        # 5. blend
        h = acc / S[..., None]
        N = np.minimum(h[..., 3] + f(1), f(max_history))
        alpha = f(1) / N
        blended = h[..., :3] + alpha[..., None] * (c - h[..., :3])
    history[has, :3] = blended[has]
    history[has, 3] = N[has]
    undecided = hit & ((np.abs(s) <= MARGIN) | (np.abs(den) <= MARGIN * (abs(prv["near"]) + abs(prv["far"]))))
    undecided |= ok2 & ((np.abs(dx - SNAP) <= MARGIN * SNAP) | (np.abs(dy - SNAP) <= MARGIN * SNAP))
    undecided |= near | (inr & (np.abs(S - MIN_WEIGHT) <= MARGIN * MIN_WEIGHT))
    return {"history": history.astype(f), "motion": motion, "has_history": has, "decidable": ~undecided}


# ---------------------------------------------------------------------------------------------------------------------
# The geometry cases
# ---------------------------------------------------------------------------------------------------------------------
def _mixed(position, look, fov=40.0) -> abi.InputStruct:
    return scenes.camera_inputs(position, scenes.normalized(look), fov)


TEMPORAL_CASES = ("translate", "rotate", "zoom", "large", "c2", "rest_mixed", "rest_planes")
MOVING_CASES = TEMPORAL_CASES[:5]
RESTING_CASES = TEMPORAL_CASES[5:]


def _identity_inputs() -> abi.InputStruct:
    return _mixed((1.2, 0.9, 7.5), (-0.18, -0.12, -1.0))


def _noise(rng, height: int, width: int) -> tuple:
    """(colour (H, W, 4), history (H, W, 4)): gamma noise, history lengths 0..39."""
    color = np.ones((height, width, 4), dtype=F)
    color[..., :3] = rng.gamma(2.0, 0.5, (height, width, 3)).astype(F)
    hist = np.zeros((height, width, 4), dtype=F)
    hist[..., :3] = rng.gamma(2.0, 0.5, (height, width, 3)).astype(F)
    hist[..., 3] = rng.integers(0, 40, (height, width)).astype(F)
    return color, hist


@functools.lru_cache(maxsize=None)
def temporal_case(name: str) -> dict:
    """The case's planes, cameras and its float64 / float32 references; computed once per process, read-only."""
    base = gbuffer_case("c2" if name == "c2" else "mixed")
    prev_inputs = base["inputs"]
    width, height = base["width"], base["height"]
    prev = base["ref"]
    if name == "rest_planes":  # identical cameras: any depth plane is consistent with itself
        p = synthetic_planes()
        height, width = p["prim_id"].shape
        prev = cur = {"normal_depth": p["normal_depth"], "prim_id": p["prim_id"]}
        inputs = prev_inputs = _identity_inputs()
    elif name == "rest_mixed":
        cur, inputs = prev, prev_inputs
    else:
        if name == "c2":
            cfg = scenes.CONFIGS["c2"]
            inputs = scenes.camera_inputs((13.0, 2.2, 3.3), cfg.orientation, cfg.fov)
        else:
            inputs = {"translate": _mixed((1.5, 1.0, 7.3), (-0.18, -0.12, -1.0)),
                      "rotate": _mixed((1.2, 0.9, 7.5), (-0.10, -0.12, -1.0)),
                      "zoom": _mixed((1.2, 0.9, 7.5), (-0.18, -0.12, -1.0), 34.0),
                      "large": _mixed((3.2, 1.4, 6.5), (-0.4, -0.15, -1.0))}[name]
        cur = gbuffer_reference(base["scene"], inputs, width, height)
    color, hist = _noise(np.random.default_rng(TEMPORAL_CASES.index(name) + 11), height, width)
    case = {"color": color, "normal_depth": np.array(cur["normal_depth"]), "prim_id": np.array(cur["prim_id"]),
            "prev_history": hist, "prev_normal_depth": np.array(prev["normal_depth"]),
            "prev_prim_id": np.array(prev["prim_id"])}
    for a in case.values():
        a.setflags(write=False)
    args = tuple(case[k] for k in ("color", "normal_depth", "prim_id", "prev_history", "prev_normal_depth", "prev_prim_id"))
    case.update(inputs=inputs, prev_inputs=prev_inputs, width=width, height=height,
                ref64=temporal_reference(*args, inputs, prev_inputs, **DEFAULTS, dtype=np.float64),
                ref32=temporal_reference(*args, inputs, prev_inputs, **DEFAULTS, dtype=np.float32))
    for r in (case["ref64"], case["ref32"]):
        for a in r.values():
            a.setflags(write=False)
    return case


def spread(case: dict, key: str) -> float:
    """d: the largest float32-vs-float64 difference of the reference on the case's decidable pixels."""
    m = case["ref64"]["decidable"]
    return float(np.abs(case["ref32"][key].astype(np.float64) - case["ref64"][key])[m].max())


# ---------------------------------------------------------------------------------------------------------------------
# The six-frame sequence (C5 at E2E_SIZE, 1 spp, the scripted orbit at 1 degree per frame)
# ---------------------------------------------------------------------------------------------------------------------
SEQUENCE_FRAMES = 6
DENOISE_DEFAULTS = (3, 0.6, 0.1, 0.05, abi.RT_DENOISE_DEMODULATE)


def sequence_inputs(k: int, frames: int = 360) -> abi.InputStruct:
    pos, fwd = scenes.moving_camera(k, frames)
    return scenes.camera_inputs(pos, fwd, end_to_end_frame()["cfg"].fov)


@functools.lru_cache(maxsize=None)
def sequence_reference() -> np.ndarray:
    """The oracle's 1024-spp radiance of the sequence's last frame."""
    e = end_to_end_frame()
    w, h = E2E_SIZE
    ref = po.render(po.OracleScene(e["scene"]), w, h, 1024, e["cfg"].depth, sequence_inputs(SEQUENCE_FRAMES - 1),
                    po.init_states(w, h, seed_base=99), radiance=True)[1]
    ref.setflags(write=False)
    return ref


def numpy_sequence(frames, gbuffers) -> dict:
    """The definition run over a sequence: frames[k] the 1-spp radiance, gbuffers[k] the planes of frame k.  Returns the
    last history plane and the filter's output on it and on the last raw frame (float32 runs)."""
    hist = None
    for k, (col, g) in enumerate(zip(frames, gbuffers)):
        if k == 0:
            hist = temporal_reference(col, g["normal_depth"], g["prim_id"], None, None, None, sequence_inputs(0), None,
                                      flags=abi.RT_TEMPORAL_RESET, dtype=np.float32)["history"]
        else:
            p = gbuffers[k - 1]
            hist = temporal_reference(col, g["normal_depth"], g["prim_id"], hist, p["normal_depth"], p["prim_id"],
                                      sequence_inputs(k), sequence_inputs(k - 1), **DEFAULTS, dtype=np.float32)["history"]
    g = gbuffers[-1]
    planes = (g["normal_depth"], g["albedo"], g["prim_id"]) + DENOISE_DEFAULTS
    return {"history": hist, "temporal_filtered": filter_reference(hist, *planes, dtype=np.float32),
            "filtered": filter_reference(frames[-1], *planes, dtype=np.float32)}


@functools.lru_cache(maxsize=None)
def oracle_sequence() -> tuple:
    """(frames, gbuffers) of the sequence from the oracle (XORWOW states carried across frames) and gbuffer_reference."""
    e = end_to_end_frame()
    w, h = E2E_SIZE
    osc, st = po.OracleScene(e["scene"]), po.init_states(w, h)
    frames, gbuffers = [], []
    for k in range(SEQUENCE_FRAMES):
        frames.append(po.render(osc, w, h, 1, e["cfg"].depth, sequence_inputs(k), st, radiance=True)[1])
        gbuffers.append(gbuffer_reference(e["scene"], sequence_inputs(k), w, h))
    return frames, gbuffers


# ---------------------------------------------------------------------------------------------------------------------
# Tests
# ---------------------------------------------------------------------------------------------------------------------
def temporal_args(width=16, height=8) -> tuple:
    """Valid rt_temporal arguments over host dummies (never dereferenced: every check precedes the first device call)."""
    n = width * height
    sizes = {"color": 16, "normal_depth": 16, "prim_id": 4, "prev_history": 16, "prev_normal_depth": 16,
             "prev_prim_id": 4, "history": 16, "motion": 8, "pos": 4}
    bufs = {k: C.create_string_buffer(n * b) for k, b in sizes.items()}
    a = abi.TemporalArgs()
    for k, b in bufs.items():
        setattr(a, k, C.addressof(b))
    a.width, a.height, a.max_history = width, height, 32
    a.depth_tol, a.normal_tol = 0.05, 0.2
    a.tiling = abi.Tiling(height, 1, 0, height)
    a.inputs = a.prev_inputs = _identity_inputs()
    return a, bufs


def _rejected(rc: int, name: str) -> None:
    assert rc == -1, rc
    assert name.encode() in lib().rt_last_error()


def test_struct_layout_matches_the_header():
    assert C.sizeof(abi.TemporalArgs) == 264
    assert abi.TemporalArgs.inputs.offset == 120 and abi.TemporalArgs.prev_inputs.offset == 192
    assert "rt_temporal" in EXPORTED
    assert lib().rt_abi_version() >= 8


def test_temporal_rejects_bad_arguments():
    L = lib()
    _rejected(L.rt_temporal(None, None), "rt_temporal")
    for field in ("color", "normal_depth", "prim_id", "prev_history", "prev_normal_depth", "prev_prim_id", "history"):
        a, keep = temporal_args()
        setattr(a, field, None)
        _rejected(L.rt_temporal(C.byref(a), None), "rt_temporal")
    for field in ("color", "normal_depth", "prim_id", "history"):  # required with RT_TEMPORAL_RESET too
        a, keep = temporal_args()
        a.flags = abi.RT_TEMPORAL_RESET
        setattr(a, field, None)
        _rejected(L.rt_temporal(C.byref(a), None), "rt_temporal")
    for flags in (1 << 2, 1 << 31, 7):
        a, keep = temporal_args()
        a.flags = flags
        _rejected(L.rt_temporal(C.byref(a), None), "flags")
    for n in (0, 4097, 1 << 20):
        a, keep = temporal_args()
        a.max_history = n
        _rejected(L.rt_temporal(C.byref(a), None), "max_history")
    for field in ("depth_tol", "normal_tol"):
        for bad in (0.0, -0.5, math.nan):
            a, keep = temporal_args()
            setattr(a, field, bad)
            _rejected(L.rt_temporal(C.byref(a), None), "tol")
    for k in (0, 1):
        a, keep = temporal_args()
        a.reserved[k] = 1
        _rejected(L.rt_temporal(C.byref(a), None), "reserved")
    a, keep = temporal_args()
    a.tiling = abi.Tiling(4, 2, 0, 4)
    _rejected(L.rt_temporal(C.byref(a), None), "tiling")
    a, keep = temporal_args()
    a.tiling = abi.Tiling(8, 1, 0, 4)
    _rejected(L.rt_temporal(C.byref(a), None), "tiling")


def test_temporal_rejects_history_aliasing_prev_history():
    """The gather reads pixels other workgroups write: history overlapping prev_history, fully or partly, is refused."""
    a, keep = temporal_args()
    a.history = a.prev_history
    _rejected(lib().rt_temporal(C.byref(a), None), "alias")
    a, keep = temporal_args()
    a.history = a.prev_history + 16 * 5
    _rejected(lib().rt_temporal(C.byref(a), None), "alias")
    a, keep = temporal_args()
    a.history = a.prev_history - 16 * 5
    _rejected(lib().rt_temporal(C.byref(a), None), "alias")


def test_an_empty_frame_is_accepted_without_a_device():
    a, keep = temporal_args()
    a.width = 0
    a.tiling = abi.Tiling(8, 1, 0, 8)
    assert lib().rt_temporal(C.byref(a), None) == 0


def test_the_inverse_projection_inverts_camera_rays():
    """Step 2 against camera_rays: a point at depth t on the centre ray of pixel (x, y) projects back to (x, y) under the
    same camera, with t_exp = t."""
    inp = _identity_inputs()
    w, h = 50, 37
    o, d = camera_rays(inp, w, h, 0.5, 0.5)
    rng = np.random.default_rng(3)
    t = rng.uniform(0.5, 30.0, (h, w)).astype(F)
    nd = np.zeros((h, w, 4), dtype=F)
    nd[..., 2] = 1.0
    nd[..., 3] = t
    prim = np.zeros((h, w), dtype=np.int32)
    color, hist = _noise(rng, h, w)
    hist[..., 3] = 5.0
    r = temporal_reference(color, nd, prim, hist, nd, prim, inp, inp, **DEFAULTS)
    assert np.all(r["motion"] == 0) and r["has_history"].all()
    # and under a shifted camera the reprojected position is where camera_rays of that camera passes through P
    prev = _mixed((1.5, 1.0, 7.3), (-0.18, -0.12, -1.0))
    P = o.astype(np.float64) + t[..., None].astype(np.float64) * d
    r = temporal_reference(color, nd, prim, hist, nd, prim, inp, prev, **DEFAULTS)
    ys, xs = np.mgrid[0:h, 0:w]
    px, py = xs + r["motion"][..., 0], ys + r["motion"][..., 1]
    inside = (px > 0) & (px < w - 1) & (py > 0) & (py < h - 1)
    assert inside.mean() > 0.3
    # the ray of the previous camera through the fractional pixel (px, py) — jitter numbers 0.5 + the fractions — passes
    # through P (the snap moves a position by up to 1/256 pixel: 1e-4 of the distance at this field of view)
    picks = list(zip(*np.nonzero(inside)))[::37]
    assert len(picks) >= 10
    for y, x in picks:
        x0, y0 = int(np.floor(px[y, x])), int(np.floor(py[y, x]))
        ro, rd = camera_rays(prev, w, h, 0.5 + (px[y, x] - x0), 0.5 - (py[y, x] - y0))
        v = P[y, x] - ro[y0, x0]
        off = np.linalg.norm(np.cross(v, rd[y0, x0].astype(np.float64)))
        assert off < 2e-4 * np.linalg.norm(v), (x, y, off)


@pytest.mark.parametrize("name", TEMPORAL_CASES)
def test_undecidable_share_is_capped(name):
    case = temporal_case(name)
    r64, r32 = case["ref64"], case["ref32"]
    share = 1.0 - float(r64["decidable"].mean())
    hit = case["prim_id"] >= 0
    no_hist = float((hit & ~r64["has_history"]).sum() / max(1, hit.sum()))
    mot = float(np.abs(r64["motion"]).max())
    print(f"{name}: {case['width']}x{case['height']}, undecidable {share:.4f}, hit pixels without history {no_hist:.3f}, "
          f"largest |motion| {mot:.1f}, d history {spread(case, 'history'):.2e}, d motion {spread(case, 'motion'):.2e}")
    assert share <= UNDECIDABLE_CAP, share
    m = r64["decidable"]
    assert np.array_equal(r32["has_history"][m], r64["has_history"][m])
    assert r64["has_history"].any() and hit.any()
    if name in MOVING_CASES:
        assert (hit & ~r64["has_history"]).any() and mot > 0.5
        lengths = r64["history"][..., 3][r64["has_history"]]
        assert lengths.max() == DEFAULTS["max_history"] and lengths.min() < DEFAULTS["max_history"]


@pytest.mark.parametrize("name", RESTING_CASES)
def test_resting_camera_is_the_running_mean(name):
    """Identical cameras: motion 0 everywhere, every hit pixel reads its own pixel (one tap, weight 1), and the float32
    reference is h + (1/N)·(c − h) bit for bit; history length 0 and miss pixels get (c, 1)."""
    case = temporal_case(name)
    r = case["ref32"]
    assert np.all(r["motion"] == 0) and np.all(case["ref64"]["motion"] == 0)
    want, has = resting_expectation(case)
    assert np.array_equal(r["has_history"], has) and has.any() and (~has).any()
    assert r["history"].dtype == np.float32 and r["history"].tobytes() == want.tobytes()
    assert case["ref64"]["decidable"].all()


def resting_expectation(case: dict) -> tuple:
    """(history (H, W, 4) float32, has_history) of a resting camera, written out directly in float32."""
    c, h = case["color"][..., :3], case["prev_history"]
    has = (case["prim_id"] >= 0) & (case["prev_prim_id"] == case["prim_id"]) & (h[..., 3] > 0)
    N = np.minimum(h[..., 3] + F(1), F(DEFAULTS["max_history"])).astype(F)
    alpha = (F(1) / N).astype(F)
    out = np.ones(h.shape, dtype=F)
    out[..., :3] = np.where(has[..., None], h[..., :3] + alpha[..., None] * (c - h[..., :3]), c)
    out[..., 3] = np.where(has, N, F(1))
    return out, has


def test_reset_and_miss_pixels_pass_the_colour_through():
    case = temporal_case("translate")
    args = tuple(case[k] for k in ("color", "normal_depth", "prim_id"))
    r = temporal_reference(*args, None, None, None, case["inputs"], None, flags=abi.RT_TEMPORAL_RESET, dtype=np.float32)
    assert r["history"][..., :3].tobytes() == case["color"][..., :3].tobytes()
    assert np.all(r["history"][..., 3] == 1) and not r["motion"].any() and not r["has_history"].any()
    case = temporal_case("c2")  # (the scene with sky)
    miss = case["prim_id"] < 0
    assert miss.any()
    r = case["ref32"]
    assert r["history"][..., :3][miss].tobytes() == case["color"][..., :3][miss].tobytes()
    assert np.all(r["history"][..., 3][miss] == 1) and not r["motion"][miss].any()
    # the colour as a sum: rgb / w, 0 where w = 0
    p = synthetic_planes()
    r = temporal_reference(p["accum"], p["normal_depth"], p["prim_id"], None, None, None, case["inputs"], None,
                           flags=abi.RT_TEMPORAL_RESET | abi.RT_TEMPORAL_COLOR_IS_SUM, dtype=np.float32)
    assert not r["history"][0, 0:4, :3].any()
    assert np.array_equal(r["history"][5, 5, :3], p["accum"][5, 5, :3] / p["accum"][5, 5, 3])


def test_the_sequence_lowers_the_error():
    """C5 at 64x48, 1 spp, depth 4, six frames of the orbit at 1 degree per frame: against the oracle's 1024-spp radiance
    of the last frame, temporal accumulation followed by the filter beats the filter alone and the raw frame."""
    frames, gbuffers = oracle_sequence()
    out = numpy_sequence(frames, gbuffers)
    ref = sequence_reference()
    raw, filt = mse(frames[-1], ref), mse(out["filtered"], ref)
    temp, both = mse(out["history"], ref), mse(out["temporal_filtered"], ref)
    print(f"sequence: mse raw {raw:.5f}, filter alone {filt:.5f}, temporal alone {temp:.5f}, temporal then filter {both:.5f}")
    assert both < filt and both < raw
    assert temp < raw
