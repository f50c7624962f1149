"""rt_scene_motion, rt_temporal_dynamic and rt_scene_edit without a device: rt_scene_motion's rules, the entry points'
argument checks, and temporal_dynamic_reference, the numpy restatement of rt_temporal_dynamic's definition
(include/rt_hip.h) that the GPU tests (test_gpu_dynamic.py) import.

temporal_dynamic_reference is temporal_reference (test_temporal_host.py) restated in full with step 1a between steps 1
and 2: m = prim_motion[prim_id]; an id beyond the table or m.s == 0 means no history; m == (0, 0, 0, 1) leaves the world
point as it is; otherwise P~ = s·P + o (a multiply, then an add, in the evaluation's type).  The decidable mask is
temporal_reference's, with the margins of s and den applied to the pixels that reach step 2.

The three object cases edit mixed_scene() (test_denoise_host.py) at 50x37: the previous planes are gbuffer_case("mixed"),
the current ones gbuffer_reference of the edited scene; colour and history are test_temporal_host._noise.  The six-frame
sequence drags two spheres of the C5 scene under the scripted orbit and compares three ways to treat the history."""
from __future__ import annotations

import ctypes as C
import functools
import math

import numpy as np
import pytest

from cudaraytracer_amd import abi, scenes
from cudaraytracer_amd._lib import EXPORTED, lib
from oracle import py_oracle as po

from test_denoise_host import (E2E_SIZE, UNDECIDABLE_CAP, end_to_end_frame, filter_reference, gbuffer_case,
                               gbuffer_reference, mixed_scene, mse)
from test_temporal_host import (DEFAULTS, DENOISE_DEFAULTS, MARGIN, MIN_WEIGHT, SEQUENCE_FRAMES, SNAP, _camera, _dot,
                                _identity_inputs, _mixed, _noise, _ray_start, sequence_inputs, temporal_args,
                                temporal_case, temporal_reference)

F = np.float32
PLANES = ("color", "normal_depth", "prim_id", "prev_history", "prev_normal_depth", "prev_prim_id")


# ---------------------------------------------------------------------------------------------------------------------
# The definition in numpy
# ---------------------------------------------------------------------------------------------------------------------
def temporal_dynamic_reference(color, normal_depth, prim_id, prev_history, prev_normal_depth, prev_prim_id, inputs,
                               prev_inputs, prim_motion, max_history=32, depth_tol=0.05, normal_tol=0.2, flags=0,
                               dtype=np.float64) -> dict:
    """history (H, W, 4), motion (H, W, 2) of `dtype`, has_history (H, W) and decidable (H, W) of rt_temporal_dynamic.
    prim_motion is the (num_prims, 4) float32 table the kernel reads (None with RT_TEMPORAL_RESET)."""
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
    table = np.asarray(prim_motion, dtype=F).reshape(-1, 4)
    num_prims = table.shape[0]
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
        # 1a. the hittable's motion entry
        in_table = (prim >= 0) & (prim < num_prims)
        if num_prims:
            m = table[np.clip(prim, 0, num_prims - 1)].astype(f)
        else:
            m = np.zeros((hgt, wid, 4), dtype=f)
        live = in_table & (m[..., 3] != 0)
        identity = (m[..., 0] == 0) & (m[..., 1] == 0) & (m[..., 2] == 0) & (m[..., 3] == 1)
        moved = m[..., 3:4] * P
        moved = moved + m[..., :3]
        P = np.where(identity[..., None], P, moved).astype(f)
        # 2. the inverse of the ray construction under the previous camera
        q = P - prv["origin"]
        a, b = _dot(q, prv["right"][None, None]), _dot(q, prv["up"][None, None])
        cf = _dot(q, prv["fw"][None, None]) / prv["ff"]
        s = (cf - prv["fov"]) / (prv["k10"] - prv["fov"])
        den = prv["near"] + s * (prv["far"] - prv["near"])
        ok2 = live & (s > 0) & (den > 0)
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
    undecided = live & ((np.abs(s) <= MARGIN) | (np.abs(den) <= MARGIN * (abs(prv["near"]) + abs(prv["far"]))))
    undecided |= ok2 & ((np.abs(dx - SNAP) <= MARGIN * SNAP) | (np.abs(dy - SNAP) <= MARGIN * SNAP))
    undecided |= near | (inr & (np.abs(S - MIN_WEIGHT) <= MARGIN * MIN_WEIGHT))
    return {"history": history.astype(f), "motion": motion, "has_history": has, "decidable": ~undecided}


def identity_table(n: int) -> np.ndarray:
    t = np.zeros((n, 4), dtype=F)
    t[:, 3] = 1.0
    return t


# ---------------------------------------------------------------------------------------------------------------------
# The object cases
# ---------------------------------------------------------------------------------------------------------------------
DYNAMIC_CASES = ("object_translate", "object_scale", "object_and_camera")
MOVED = {"object_translate": (2, 6), "object_scale": (0, 7), "object_and_camera": (0, 2, 5, 6, 7)}
CROP_SIZE = (70, 9)  # the partial-tile frame of the GPU tests: neither a multiple of 64 wide nor of 4 high


def edited_mixed_scene(name: str) -> scenes.Scene:
    s = mixed_scene()
    h = s.hittables

    def move(i, dx=0.0, dy=0.0, dz=0.0):
        h[i].center[0] += dx
        h[i].center[1] += dy
        h[i].center[2] += dz

    if name in ("object_translate", "object_and_camera"):
        move(2, 0.15, 0.05, -0.1)
        move(6, dx=-0.2)
    if name in ("object_scale", "object_and_camera"):
        h[0].radius = 0.9
        h[7].radius = 1.2
        h[7].center[1] = 0.2
    if name == "object_and_camera":
        h[8].is_active = 0
        move(5, dz=0.3)
    return s


def _build_case(name: str, width: int, height: int, prev: dict, prev_inputs, seed: int) -> dict:
    scene = edited_mixed_scene(name)
    inputs = _mixed((1.5, 1.0, 7.3), (-0.18, -0.12, -1.0)) if name == "object_and_camera" else prev_inputs
    cur = gbuffer_reference(scene, inputs, width, height)
    table = scenes.scene_motion(mixed_scene(), scene)
    color, hist = _noise(np.random.default_rng(seed), height, width)
    case = {"color": color, "normal_depth": np.array(cur["normal_depth"]), "prim_id": np.array(cur["prim_id"]),
            "prev_history": hist, "prev_normal_depth": np.array(prev["normal_depth"]),
            "prev_prim_id": np.array(prev["prim_id"]), "prim_motion": table}
    for a in case.values():
        a.setflags(write=False)
    args = tuple(case[k] for k in PLANES)
    case.update(inputs=inputs, prev_inputs=prev_inputs, width=width, height=height, scene=scene,
                moved=np.isin(case["prim_id"], MOVED[name]),
                ref64=temporal_dynamic_reference(*args, inputs, prev_inputs, table, **DEFAULTS, dtype=np.float64),
                ref32=temporal_dynamic_reference(*args, inputs, prev_inputs, table, **DEFAULTS, dtype=np.float32),
                static64=temporal_dynamic_reference(*args, inputs, prev_inputs, identity_table(len(table)), **DEFAULTS,
                                                    dtype=np.float64))
    for r in (case["ref64"], case["ref32"], case["static64"]):
        for a in r.values():
            a.setflags(write=False)
    return case


@functools.lru_cache(maxsize=None)
def dynamic_case(name: str) -> dict:
    """The case's planes, cameras, motion table and its float64 / float32 references; computed once, read-only."""
    base = gbuffer_case("mixed")
    return _build_case(name, base["width"], base["height"], base["ref"], base["inputs"], 31 + DYNAMIC_CASES.index(name))


@functools.lru_cache(maxsize=None)
def crop_case() -> dict:
    """object_and_camera's scene, edits and cameras at CROP_SIZE, both frames' planes from gbuffer_reference."""
    base = gbuffer_case("mixed")
    w, h = CROP_SIZE
    prev = gbuffer_reference(base["scene"], base["inputs"], w, h)
    return _build_case("object_and_camera", w, h, prev, base["inputs"], 47)


def spread(case: dict, key: str) -> float:
    """d: the largest float32-vs-float64 difference of the reference on the case's decidable pixels."""
    m = case["ref64"]["decidable"]
    return float(np.abs(case["ref32"][key].astype(np.float64) - case["ref64"][key])[m].max())


# ---------------------------------------------------------------------------------------------------------------------
# The six-frame moving-object sequence (C5 at E2E_SIZE, 1 spp, the scripted orbit, two spheres dragged)
# ---------------------------------------------------------------------------------------------------------------------
SEQUENCE_MOVED = (2, 4)


def sequence_scene(k: int) -> scenes.Scene:
    """Frame k's scene: hittable 4 at (1.5 − 0.08·k, 0, 2.5 + 0.03·k), hittable 2 at y = 0.5 + 0.05·k."""
    cfg = end_to_end_frame()["cfg"]
    s = cfg.scene_desc()
    s.hittables[4].center[:] = [1.5 - 0.08 * k, 0.0, 2.5 + 0.03 * k]
    s.hittables[2].center[1] = 0.5 + 0.05 * k
    return s


def sequence_table(k: int) -> np.ndarray:
    return scenes.scene_motion(sequence_scene(k - 1), sequence_scene(k))


@functools.lru_cache(maxsize=None)
def dynamic_sequence_reference() -> np.ndarray:
    """The oracle's 1024-spp radiance of the last frame's scene under the last camera."""
    cfg = end_to_end_frame()["cfg"]
    w, h = E2E_SIZE
    ref = po.render(po.OracleScene(sequence_scene(SEQUENCE_FRAMES - 1)), w, h, 1024, cfg.depth,
                    sequence_inputs(SEQUENCE_FRAMES - 1), po.init_states(w, h, seed_base=99), radiance=True)[1]
    ref.setflags(write=False)
    return ref


@functools.lru_cache(maxsize=None)
def oracle_dynamic_sequence() -> tuple:
    """(frames, gbuffers) of the sequence from the oracle (XORWOW states carried across frames) and gbuffer_reference."""
    cfg = end_to_end_frame()["cfg"]
    w, h = E2E_SIZE
    st = po.init_states(w, h)
    frames, gbuffers = [], []
    for k in range(SEQUENCE_FRAMES):
        scene = sequence_scene(k)
        frames.append(po.render(po.OracleScene(scene), w, h, 1, cfg.depth, sequence_inputs(k), st, radiance=True)[1])
        gbuffers.append(gbuffer_reference(scene, sequence_inputs(k), w, h))
    return frames, gbuffers


def numpy_dynamic_sequence(frames, gbuffers) -> dict:
    """The three history handlings over the sequence (float32 runs): per handling the last history plane and the
    filter's output on it.  "reset": every frame restarts (the last raw frame); "ignored": rt_temporal's definition, the
    objects' motion unknown to it; "table": rt_temporal_dynamic's with rt_scene_motion's table."""
    hist = {"ignored": None, "table": None}
    for k, (col, g) in enumerate(zip(frames, gbuffers)):
        cur = (col, g["normal_depth"], g["prim_id"])
        if k == 0:
            first = temporal_reference(*cur, None, None, None, sequence_inputs(0), None, flags=abi.RT_TEMPORAL_RESET,
                                       dtype=np.float32)["history"]
            hist = {"ignored": first, "table": first}
            continue
        p = gbuffers[k - 1]
        cams = (sequence_inputs(k), sequence_inputs(k - 1))
        hist["ignored"] = temporal_reference(*cur, hist["ignored"], p["normal_depth"], p["prim_id"], *cams, **DEFAULTS,
                                             dtype=np.float32)["history"]
        hist["table"] = temporal_dynamic_reference(*cur, hist["table"], p["normal_depth"], p["prim_id"], *cams,
                                                   sequence_table(k), **DEFAULTS, dtype=np.float32)["history"]
    g = gbuffers[-1]
    hist["reset"] = temporal_reference(frames[-1], g["normal_depth"], g["prim_id"], None, None, None,
                                       sequence_inputs(SEQUENCE_FRAMES - 1), None, flags=abi.RT_TEMPORAL_RESET,
                                       dtype=np.float32)["history"]
    planes = (g["normal_depth"], g["albedo"], g["prim_id"]) + DENOISE_DEFAULTS
    out = {}
    for key, plane in hist.items():
        out[key] = plane
        out[key + "_filtered"] = filter_reference(plane, *planes, dtype=np.float32)
    return out


def sequence_errors(out: dict, gbuffers, ref) -> dict:
    """Mean squared errors against the oracle: whole frame per handling (temporal, temporal + filter) and, on the moved
    objects' pixels of the last frame, of the temporal planes."""
    moved = np.isin(gbuffers[-1]["prim_id"], SEQUENCE_MOVED)
    err = {"moved_pixels": int(moved.sum())}
    for key in ("reset", "ignored", "table"):
        err[key] = mse(out[key], ref)
        err[key + "_filtered"] = mse(out[key + "_filtered"], ref)
        err[key + "_moved"] = mse(np.asarray(out[key])[moved], np.asarray(ref)[moved])
    return err


def assert_sequence_orderings(err: dict) -> None:
    assert err["moved_pixels"] > 0
    assert err["table"] < err["reset"]
    assert err["table_filtered"] < err["reset_filtered"]
    assert err["table_moved"] < err["ignored_moved"]


def format_errors(err: dict) -> str:
    rows = [f"{key}: temporal {err[key]:.5f}, + filter {err[key + '_filtered']:.5f}, moved objects {err[key + '_moved']:.5f}"
            for key in ("reset", "ignored", "table")]
    return f"{err['moved_pixels']} moved-object pixels; " + "; ".join(rows)


# ---------------------------------------------------------------------------------------------------------------------
# Tests: exports, rt_scene_motion
# ---------------------------------------------------------------------------------------------------------------------
def test_exports_and_version():
    for name in ("rt_scene_motion", "rt_temporal_dynamic", "rt_scene_edit"):
        assert name in EXPORTED
        assert hasattr(lib(), name)
    assert lib().rt_abi_version() >= 9
    assert C.sizeof(abi.TemporalArgs) == 264  # (the new call takes rt_temporal's structure unchanged)


def _hittable(ty, center, radius=0.0, width=0.0, height=0.0, active=1, material=0) -> abi.HittableDesc:
    h = abi.HittableDesc()
    h.type, h.is_active, h.material = ty, active, material
    h.center[:] = list(center)
    h.radius, h.width, h.height = radius, width, height
    return h


def _motion(prev: abi.HittableDesc, cur: abi.HittableDesc) -> np.ndarray:
    t = scenes.scene_motion([prev], [cur])
    assert t.shape == (1, 4) and t.dtype == np.float32
    return t[0]


def test_scene_motion_of_a_translated_sphere():
    cp, cc = np.array([1.1, -0.35, 0.6], dtype=F), np.array([1.25, -0.3, 0.5], dtype=F)
    m = _motion(_hittable(abi.RT_SPHERE, cp, 0.65), _hittable(abi.RT_SPHERE, cc, 0.65))
    assert m[3] == F(1.0)
    assert m[:3].tobytes() == (cp - cc).astype(F).tobytes()


def test_scene_motion_of_a_resized_sphere():
    cp, cc = np.array([-1.3, 0.0, -0.4], dtype=F), np.array([-1.3, 0.25, -0.4], dtype=F)
    s = F(1.0) / F(0.9)
    for centre in (cp, cc):  # the radius alone, and the radius with the centre
        m = _motion(_hittable(abi.RT_SPHERE, cp, 1.0), _hittable(abi.RT_SPHERE, centre, 0.9))
        assert m[3].tobytes() == s.tobytes()
        want = (cp - (s * centre).astype(F)).astype(F)
        assert m[:3].tobytes() == want.tobytes()
    assert s != F(1.0)


@pytest.mark.parametrize("ty", [abi.RT_XYRECT, abi.RT_XZRECT, abi.RT_YZRECT])
def test_scene_motion_of_a_moved_rectangle(ty):
    cp, cc = np.array([1.0, 2.6, -1.0], dtype=F), np.array([0.8, 2.6, -1.3], dtype=F)
    m = _motion(_hittable(ty, cp, width=2.0, height=3.0), _hittable(ty, cc, width=2.0, height=3.0))
    assert m[3] == F(1.0)
    assert m[:3].tobytes() == (cp - cc).astype(F).tobytes()


def test_scene_motion_without_history():
    c = (0.5, 0.25, -1.0)
    sphere, rect = _hittable(abi.RT_SPHERE, c, 1.0), _hittable(abi.RT_XZRECT, c, width=2.0, height=3.0)
    none = np.zeros(4, dtype=F).tobytes()
    cases = {
        "rectangle wider": (rect, _hittable(abi.RT_XZRECT, c, width=2.5, height=3.0)),
        "rectangle higher": (rect, _hittable(abi.RT_XZRECT, c, width=2.0, height=3.5)),
        "type changed": (rect, _hittable(abi.RT_XYRECT, c, width=2.0, height=3.0)),
        "sphere to rectangle": (sphere, _hittable(abi.RT_XZRECT, c, 1.0, 2.0, 3.0)),
        "previous inactive": (_hittable(abi.RT_SPHERE, c, 1.0, active=0), sphere),
        "current inactive": (sphere, _hittable(abi.RT_SPHERE, c, 1.0, active=0)),
        "radius 0 now": (sphere, _hittable(abi.RT_SPHERE, c, 0.0)),
        "radius 0 before": (_hittable(abi.RT_SPHERE, c, 0.0), sphere),
    }
    for what, (prev, cur) in cases.items():
        assert _motion(prev, cur).tobytes() == none, what


def test_scene_motion_of_an_unchanged_hittable_is_the_identity():
    ident = np.array(abi.MOTION_IDENTITY, dtype=F).tobytes()
    for h in (_hittable(abi.RT_SPHERE, (1.1, -0.35, 0.6), 0.65), _hittable(abi.RT_YZRECT, (-3.5, 1.5, 0.0), width=9.0, height=5.0),
              _hittable(abi.RT_SPHERE, (-0.0, 1e30, -7.0), 3.0)):
        assert _motion(h, h).tobytes() == ident
    # a material change is the caller's to handle: the entry stays the identity
    a, b = _hittable(abi.RT_SPHERE, (1.0, 2.0, 3.0), 1.0, material=0), _hittable(abi.RT_SPHERE, (1.0, 2.0, 3.0), 1.0, material=1)
    assert _motion(a, b).tobytes() == ident
    # a whole scene against itself, and against its edit
    s = mixed_scene()
    assert scenes.scene_motion(s, s).tobytes() == identity_table(s.num_hittables).tobytes()
    t = scenes.scene_motion(s, edited_mixed_scene("object_and_camera"))
    rest = [i for i in range(s.num_hittables) if i not in MOVED["object_and_camera"] and i != 8]
    assert t[rest].tobytes() == identity_table(len(rest)).tobytes()
    assert not t[8].any() and all(t[i, 3] != 0 and t[i, :3].any() for i in MOVED["object_and_camera"])


def test_scene_motion_rejects_bad_arguments():
    L = lib()
    h = (abi.HittableDesc * 2)()
    t = (C.c_float * 8)()
    for args in ((None, h, 2, t), (h, None, 2, t), (h, h, 2, None)):
        assert L.rt_scene_motion(*args) == -1
        assert b"rt_scene_motion" in L.rt_last_error()
    assert L.rt_scene_motion(None, None, 0, None) == 0
    with pytest.raises(ValueError):
        scenes.scene_motion(mixed_scene(), [_hittable(abi.RT_SPHERE, (0, 0, 0), 1.0)])


# ---------------------------------------------------------------------------------------------------------------------
# Tests: the reference
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["translate", "rest_mixed"])
def test_identity_table_is_temporal_reference(name):
    case = temporal_case(name)
    args = tuple(case[k] for k in PLANES) + (case["inputs"], case["prev_inputs"])
    table = identity_table(int(case["prim_id"].max()) + 1)
    for dtype, key in ((np.float64, "ref64"), (np.float32, "ref32")):
        r = temporal_dynamic_reference(*args, table, **DEFAULTS, dtype=dtype)
        for plane in ("history", "motion", "has_history", "decidable"):
            assert r[plane].dtype == case[key][plane].dtype and r[plane].tobytes() == case[key][plane].tobytes(), (dtype, plane)


@pytest.mark.parametrize("name", DYNAMIC_CASES)
def test_object_cases_on_the_reference(name):
    case = dynamic_case(name)
    r64, r32, st = case["ref64"], case["ref32"], case["static64"]
    share = 1.0 - float(r64["decidable"].mean())
    m = r64["decidable"]
    moved = case["moved"]
    with_history = int((moved & r64["has_history"]).sum())
    differs = int((moved & np.any(r64["history"] != st["history"], axis=-1)).sum())
    print(f"{name}: {case['width']}x{case['height']}, undecidable {share:.4f}, moved-object pixels {int(moved.sum())}, with "
          f"history {with_history}, differing from the identity table's result {differs}, largest |motion| on them "
          f"{float(np.abs(r64['motion'][moved]).max()):.2f}, d history {spread(case, 'history'):.2e}, d motion "
          f"{spread(case, 'motion'):.2e}")
    assert share <= UNDECIDABLE_CAP, share
    assert np.array_equal(r32["has_history"][m], r64["has_history"][m])
    assert moved.sum() > 0
    assert with_history > moved.sum() / 2
    # a kernel that ignores the table cannot pass: on most of the moved objects' pixels the result differs from the
    # identity table's, and the motion planes differ
    assert differs > moved.sum() / 2
    assert np.any(r64["motion"][moved] != st["motion"][moved])
    # pixels of resting hittables are the identity table's
    rest = ~moved
    assert r64["history"][rest].tobytes() == st["history"][rest].tobytes()
    assert r64["motion"][rest].tobytes() == st["motion"][rest].tobytes()


def test_crop_case_on_the_reference():
    case = crop_case()
    assert (case["width"], case["height"]) == CROP_SIZE and case["width"] % 64 and case["height"] % 4
    assert 1.0 - float(case["ref64"]["decidable"].mean()) <= UNDECIDABLE_CAP
    assert case["moved"].any() and (case["moved"] & case["ref64"]["has_history"]).any()


def test_a_zero_entry_means_no_history():
    case = dynamic_case("object_translate")
    args = tuple(case[k] for k in PLANES) + (case["inputs"], case["prev_inputs"])
    table = np.array(case["prim_motion"])
    table[1] = 0.0  # the floor
    floor = case["prim_id"] == 1
    assert floor.any() and case["ref32"]["has_history"][floor].any()
    for cut in (table, table[:1]):  # a zero entry, and a table that ends before the id
        r = temporal_dynamic_reference(*args, cut, **DEFAULTS, dtype=np.float32)
        assert r["history"][..., :3][floor].tobytes() == case["color"][..., :3][floor].tobytes()
        assert np.all(r["history"][..., 3][floor] == 1) and not r["motion"][floor].any() and not r["has_history"][floor].any()
    r = temporal_dynamic_reference(*args, table, **DEFAULTS, dtype=np.float32)
    assert r["history"][~floor].tobytes() == case["ref32"]["history"][~floor].tobytes()


def test_the_motion_table_lowers_the_error_of_the_sequence():
    """C5 at 64x48, 1 spp, depth 4, six frames of the orbit while hittables 4 and 2 are dragged.  Against the oracle's
    1024-spp radiance of the last scene: history carried through the motion table beats restarting every frame on the
    whole frame (with and without the filter), and beats ignoring the motion on the moved objects' pixels."""
    frames, gbuffers = oracle_dynamic_sequence()
    err = sequence_errors(numpy_dynamic_sequence(frames, gbuffers), gbuffers, dynamic_sequence_reference())
    print("numpy pipeline: " + format_errors(err))
    assert_sequence_orderings(err)


# ---------------------------------------------------------------------------------------------------------------------
# Tests: argument checks
# ---------------------------------------------------------------------------------------------------------------------
def dynamic_args(width=16, height=8, num_prims=4) -> tuple:
    """Valid rt_temporal_dynamic arguments over host dummies (never dereferenced: every check precedes the launch)."""
    a, bufs = temporal_args(width, height)
    raw = C.create_string_buffer(16 * num_prims + 16)
    bufs["prim_motion_raw"] = raw
    table = (C.addressof(raw) + 15) & ~15
    return a, table, num_prims, bufs


def _rejected(rc: int, name: str) -> None:
    assert rc == -1, rc
    assert name.encode() in lib().rt_last_error()


def test_dynamic_rejects_a_missing_or_overlapping_table():
    L = lib()
    a, table, n, keep = dynamic_args()
    _rejected(L.rt_temporal_dynamic(C.byref(a), None, n, None), "prim_motion")
    _rejected(L.rt_temporal_dynamic(C.byref(a), table + 4, n, None), "prim_motion")  # not a float4 address
    for field, stride in (("history", 16), ("motion", 8), ("pos", 4)):
        a, table, n, keep = dynamic_args()
        out = getattr(a, field)
        for at in (out, out + 16 * 3, out + stride * 16 * 8 - 16):  # the start, inside, the last 16 bytes
            _rejected(L.rt_temporal_dynamic(C.byref(a), at, n, None), "prim_motion")
        _rejected(L.rt_temporal_dynamic(C.byref(a), out - 16, 2, None), "prim_motion")  # the table's tail reaches in
    # with RT_TEMPORAL_RESET the table is never read: NULL is accepted up to the launch, which needs a device
    a, table, n, keep = dynamic_args()
    a.flags = abi.RT_TEMPORAL_RESET
    a.width = 0
    assert L.rt_temporal_dynamic(C.byref(a), None, 0, None) == 0


def test_dynamic_rejects_what_temporal_rejects():
    L = lib()

    def call(a, table, n):
        return L.rt_temporal_dynamic(C.byref(a), table, n, None)

    _rejected(L.rt_temporal_dynamic(None, None, 0, None), "rt_temporal_dynamic")
    for field in ("color", "normal_depth", "prim_id", "prev_history", "prev_normal_depth", "prev_prim_id", "history"):
        a, table, n, keep = dynamic_args()
        setattr(a, field, None)
        _rejected(call(a, table, n), "rt_temporal_dynamic")
    for field in ("color", "normal_depth", "prim_id", "history"):  # required with RT_TEMPORAL_RESET too
        a, table, n, keep = dynamic_args()
        a.flags = abi.RT_TEMPORAL_RESET
        setattr(a, field, None)
        _rejected(call(a, table, n), "rt_temporal_dynamic")
    for flags in (1 << 2, 1 << 31, 7):
        a, table, n, keep = dynamic_args()
        a.flags = flags
        _rejected(call(a, table, n), "flags")
    for count in (0, 4097, 1 << 20):
        a, table, n, keep = dynamic_args()
        a.max_history = count
        _rejected(call(a, table, n), "max_history")
    for field in ("depth_tol", "normal_tol"):
        for bad in (0.0, -0.5, math.nan):
            a, table, n, keep = dynamic_args()
            setattr(a, field, bad)
            _rejected(call(a, table, n), "tol")
    for k in (0, 1):
        a, table, n, keep = dynamic_args()
        a.reserved[k] = 1
        _rejected(call(a, table, n), "reserved")
    for tiling in (abi.Tiling(4, 2, 0, 4), abi.Tiling(8, 1, 0, 4)):
        a, table, n, keep = dynamic_args()
        a.tiling = tiling
        _rejected(call(a, table, n), "tiling")
    for offset in (0, 16 * 5, -16 * 5):  # history aliasing prev_history, fully or partly
        a, table, n, keep = dynamic_args()
        a.history = a.prev_history + offset
        _rejected(call(a, table, n), "alias")


def test_dynamic_accepts_an_empty_frame_without_a_device():
    a, table, n, keep = dynamic_args()
    a.width = 0
    a.tiling = abi.Tiling(8, 1, 0, 8)
    assert lib().rt_temporal_dynamic(C.byref(a), table, n, None) == 0
    _rejected(lib().rt_temporal_dynamic(C.byref(a), None, n, None), "prim_motion")  # (the checks still run)


def test_scene_edit_rejects_bad_arguments():
    """NULLs are refused before anything is read.  The count check needs a base scene, which needs a device: it runs here
    where one exists and in test_gpu_dynamic.py::test_scene_edit_rejects_a_wrong_count in any case."""
    L = lib()
    s = mixed_scene()
    out = C.c_void_p(1)
    _rejected(L.rt_scene_edit(None, s.hittables, s.num_hittables, C.byref(out)), "rt_scene_edit")
    assert not out.value  # (the out handle is cleared on failure)
    _rejected(L.rt_scene_edit(None, s.hittables, s.num_hittables, None), "rt_scene_edit")
    base = C.c_void_p()
    desc = s.desc()
    if L.rt_scene_create(C.byref(desc), C.byref(base)) != 0:
        return  # no device on this machine
    try:
        _rejected(L.rt_scene_edit(base, None, s.num_hittables, C.byref(out)), "rt_scene_edit")
        _rejected(L.rt_scene_edit(base, s.hittables, s.num_hittables - 1, C.byref(out)), "count")
        _rejected(L.rt_scene_edit(base, s.hittables, s.num_hittables + 1, C.byref(out)), "count")
        assert not out.value
    finally:
        L.rt_scene_destroy(base)
