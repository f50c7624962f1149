"""rt_temporal_dynamic and rt_scene_edit on the GPU, against the numpy restatement of the definition
(tests/test_dynamic_host.py temporal_dynamic_reference) and against rt_temporal / rt_scene_create.

Tolerance of the reference match, the rule of test_gpu_temporal.py: d = the largest absolute difference between the
reference's own float32 and float64 runs on the case's decidable pixels (history and motion each have their own d); the
kernel performs the float32 reference's operations in its order, so 4·d covers only the library's own division and square
root.  "Has history" must agree exactly on decidable pixels.  The measured ratios are recorded in DESIGN.md §13."""
from __future__ import annotations

import ctypes as C

import numpy as np
import pytest
import torch

from cudaraytracer_amd import abi, scenes
from cudaraytracer_amd._lib import lib
from cudaraytracer_amd.renderer import DeviceScene, Renderer

from test_denoise_host import E2E_SIZE, UNDECIDABLE_CAP, end_to_end_frame, mixed_scene, rgb_to_int_np
from test_dynamic_host import (CROP_SIZE, DYNAMIC_CASES, PLANES, SEQUENCE_FRAMES, assert_sequence_orderings, crop_case,
                               dynamic_case, dynamic_sequence_reference, format_errors, identity_table,
                               numpy_dynamic_sequence, sequence_errors, sequence_inputs, sequence_scene, spread)
from test_temporal_host import DEFAULTS, temporal_case

pytestmark = pytest.mark.gpu

FILL = -7.0
GUARD = 3  # rows and columns of the output tensors around the frame that no call may write


def run_pass(case: dict, table="case", num_prims=None, flags: int = 0, static: bool = False, guard: int = 0) -> tuple:
    """(history (H, W, 4) float32, motion (H, W, 2) float32, pos (H, W) uint32) of one rt_temporal_dynamic call on the
    case's planes (static: of rt_temporal).  table: "case" = the case's motion table, None = NULL, else an (n, 4) array.
    guard > 0: the outputs live in the middle rows of taller tensors filled with FILL / 0, with `guard` rows before and
    after (a row-major frame's neighbours in memory are the rows before its first and after its last pixel: a write
    outside the frame, columns past the width included, lands there); those rows are returned too."""
    dev = torch.device("cuda", 0)
    h, w = case["prim_id"].shape
    t = {k: torch.from_numpy(np.array(case[k])).to(dev) for k in PLANES}
    hist = torch.full((h + 2 * guard, w, 4), FILL, dtype=torch.float32, device=dev)
    motion = torch.full((h + 2 * guard, w, 2), FILL, dtype=torch.float32, device=dev)
    pos = torch.zeros((h + 2 * guard, w), dtype=torch.int32, device=dev)
    a = abi.TemporalArgs()
    for k, v in t.items():
        setattr(a, k, v.data_ptr())
    a.history, a.motion, a.pos = hist[guard:].data_ptr(), motion[guard:].data_ptr(), pos[guard:].data_ptr()
    a.width, a.height, a.flags, a.max_history = w, h, flags, DEFAULTS["max_history"]
    a.depth_tol, a.normal_tol = DEFAULTS["depth_tol"], DEFAULTS["normal_tol"]
    a.tiling = abi.Tiling(h, 1, 0, h)
    a.inputs, a.prev_inputs = case["inputs"], case["prev_inputs"]
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    if static:
        rc = lib().rt_temporal(C.byref(a), stream)
    else:
        if isinstance(table, str):
            table = case["prim_motion"]
        dtable = None if table is None else torch.from_numpy(np.array(table, dtype=np.float32)).to(dev)
        n = 0 if dtable is None else dtable.shape[0]
        rc = lib().rt_temporal_dynamic(C.byref(a), None if dtable is None else C.c_void_p(dtable.data_ptr()),
                                       n if num_prims is None else num_prims, stream)
    assert rc == 0, lib().rt_last_error()
    torch.cuda.synchronize()
    return hist.cpu().numpy(), motion.cpu().numpy(), pos.cpu().numpy().view(np.uint32)


def same_bits(a: tuple, b: tuple) -> bool:
    return all(x.tobytes() == y.tobytes() for x, y in zip(a, b))


@pytest.mark.parametrize("name", ["translate", "rest_mixed"])
def test_identity_table_is_rt_temporal(name):
    case = temporal_case(name)
    table = identity_table(int(case["prim_id"].max()) + 1)
    got, want = run_pass(case, table), run_pass(case, static=True)
    assert same_bits(got, want)
    assert (want[0][..., 3] > 1.0).any()


def check_against_reference(case: dict, got: tuple, label: str) -> None:
    r64 = case["ref64"]
    m = r64["decidable"]
    assert 1.0 - float(m.mean()) <= UNDECIDABLE_CAP
    hist, motion, _ = got
    for key, plane in (("history", hist), ("motion", motion)):
        d = spread(case, key)
        err = float(np.abs(plane.astype(np.float64) - r64[key])[m].max())
        print(f"{label} {key}: GPU error {err:.3e}, float32-vs-float64 spread d {d:.3e}, ratio {err / d if d else 0.0:.2f}")
        assert err <= 4 * d, (key, err, d)
    assert np.array_equal((hist[..., 3] > 1.0)[m], r64["has_history"][m])
    assert np.all(hist[..., 3] >= 1.0) and np.all(hist[..., 3] <= DEFAULTS["max_history"])
    assert np.all(motion[case["prim_id"] < 0] == 0)


@pytest.mark.parametrize("name", DYNAMIC_CASES)
def test_object_cases_match_the_reference(name):
    case = dynamic_case(name)
    got = run_pass(case)
    check_against_reference(case, got, name)
    assert (got[0][..., 3][case["moved"]] > 1.0).any()


def test_partial_tiles_write_nothing_outside_the_frame():
    """70x9: two workgroups across, the second 6 pixels wide; three down, the last one row high."""
    case = crop_case()
    w, h = CROP_SIZE
    hist, motion, pos = run_pass(case, guard=GUARD)
    for plane, fill in ((hist, FILL), (motion, FILL), (pos, 0)):
        assert plane.shape[0] == h + 2 * GUARD and plane.shape[1] == w
        assert np.all(plane[:GUARD] == fill) and np.all(plane[GUARD + h:] == fill)
    inner = (hist[GUARD:GUARD + h], motion[GUARD:GUARD + h], pos[GUARD:GUARD + h])
    assert np.all(inner[0] != FILL) and np.all(inner[1] != FILL)
    check_against_reference(case, inner, "70x9")
    assert same_bits(inner, run_pass(case))
    assert np.array_equal(inner[2], rgb_to_int_np(inner[0][..., :3]))


def test_a_short_table_means_no_history_beyond_it():
    case = dynamic_case("object_and_camera")
    ids = case["prim_id"]
    full = run_pass(case)
    cut = 5
    beyond = ids >= cut
    assert beyond.any() and (full[0][..., 3][beyond] > 1.0).any() and ids.max() >= cut
    hist, motion, pos = run_pass(case, num_prims=cut)  # the same device table, fewer entries declared
    assert hist[..., :3][beyond].tobytes() == case["color"][..., :3][beyond].tobytes()
    assert np.all(hist[..., 3][beyond] == 1.0) and not motion[beyond].any()
    for got, want in zip((hist, motion, pos), full):
        assert got[~beyond].tobytes() == want[~beyond].tobytes()
    hist, motion, _ = run_pass(case, case["prim_motion"][:cut])  # and a table that really ends there
    assert np.all(hist[..., 3][beyond] == 1.0) and hist[~beyond].tobytes() == full[0][~beyond].tobytes()
    hist, _, _ = run_pass(case, num_prims=0)
    assert np.all(hist[..., 3] == 1.0) and hist[..., :3].tobytes() == case["color"][..., :3].tobytes()


def test_a_zero_entry_means_no_history():
    case = dynamic_case("object_translate")
    table = np.array(case["prim_motion"])
    table[1] = 0.0
    floor = case["prim_id"] == 1
    full = run_pass(case)
    hist, motion, _ = run_pass(case, table)
    assert floor.any() and (full[0][..., 3][floor] > 1.0).any()
    assert hist[..., :3][floor].tobytes() == case["color"][..., :3][floor].tobytes()
    assert np.all(hist[..., 3][floor] == 1.0) and not motion[floor].any()
    assert hist[~floor].tobytes() == full[0][~floor].tobytes() and motion[~floor].tobytes() == full[1][~floor].tobytes()


def test_reset_with_a_null_table_is_rt_temporal_with_the_flag():
    case = dynamic_case("object_and_camera")
    want = run_pass(case, flags=abi.RT_TEMPORAL_RESET, static=True)
    assert same_bits(run_pass(case, None, flags=abi.RT_TEMPORAL_RESET), want)
    assert same_bits(run_pass(case, flags=abi.RT_TEMPORAL_RESET), want)
    assert want[0][..., :3].tobytes() == case["color"][..., :3].tobytes() and np.all(want[0][..., 3] == 1.0)


def test_two_calls_give_the_same_bits():
    case = dynamic_case("object_and_camera")
    assert same_bits(run_pass(case), run_pass(case))


@pytest.mark.parametrize("name", ["object_scale", "object_and_camera"])
def test_pos_is_the_render_kernels_epilogue(name):
    hist, _, pos = run_pass(dynamic_case(name))
    assert np.array_equal(pos, rgb_to_int_np(hist[..., :3]))


def test_an_overlapping_table_is_rejected_and_writes_nothing():
    dev = torch.device("cuda", 0)
    case = dynamic_case("object_translate")
    h, w = case["prim_id"].shape
    t = {k: torch.from_numpy(np.array(case[k])).to(dev) for k in PLANES}
    hist = torch.full((h, w, 4), FILL, dtype=torch.float32, device=dev)
    a = abi.TemporalArgs()
    for k, v in t.items():
        setattr(a, k, v.data_ptr())
    a.history = hist.data_ptr()
    a.width, a.height, a.max_history = w, h, 32
    a.depth_tol, a.normal_tol = 0.05, 0.2
    a.tiling = abi.Tiling(h, 1, 0, h)
    a.inputs, a.prev_inputs = case["inputs"], case["prev_inputs"]
    assert lib().rt_temporal_dynamic(C.byref(a), C.c_void_p(hist.data_ptr() + 64), 9, None) == -1
    assert b"prim_motion" in lib().rt_last_error()
    assert lib().rt_temporal_dynamic(C.byref(a), None, 9, None) == -1
    torch.cuda.synchronize()
    assert np.all(hist.cpu().numpy() == FILL)


# ---------------------------------------------------------------------------------------------------------------------
# rt_scene_edit
# ---------------------------------------------------------------------------------------------------------------------
def _render_and_gbuffer(ds: DeviceScene, cfg) -> tuple:
    """(image, RNG states, normal_depth, albedo, prim_id) of one 1-spp XORWOW frame and one G-buffer pass."""
    w, h = E2E_SIZE
    r = Renderer(w, h)
    r.render_init()
    inp = sequence_inputs(2)
    r.render(ds, 1, cfg.depth, inp)
    nd, alb, ids = r.gbuffer(ds, inp)
    torch.cuda.synchronize()
    return r.image().copy(), r.states().copy(), nd.cpu().numpy(), alb.cpu().numpy(), ids.cpu().numpy()


def test_scene_edit_equals_a_scene_created_from_scratch():
    """C5 at 64x48 with hittable 4 moved: the edited handle renders what rt_scene_create of the same description does,
    bit for bit, and the two handles outlive each other in either order."""
    cfg = end_to_end_frame()["cfg"]
    base_scene, moved_scene = sequence_scene(0), sequence_scene(3)
    scratch = DeviceScene(moved_scene)
    want = _render_and_gbuffer(scratch, cfg)
    scratch.close()
    base = DeviceScene(base_scene)
    before = _render_and_gbuffer(base, cfg)
    assert not np.array_equal(before[4], want[4])  # (the edit is visible)
    edited = base.edited(moved_scene.hittables)
    info_e, info_s = edited.info(), DeviceScene(moved_scene).info()
    assert (info_e.num_primitives, info_e.num_nodes, info_e.num_materials, info_e.bvh_depth, info_e.device_bytes) == \
           (info_s.num_primitives, info_s.num_nodes, info_s.num_materials, info_s.bvh_depth, info_s.device_bytes)
    assert same_bits(_render_and_gbuffer(edited, cfg), want)
    # the edited handle goes first: the base renders as before (the shared texels are still there)
    edited.close()
    assert same_bits(_render_and_gbuffer(base, cfg), before)
    # the base goes first: the edited handle renders as before; and an edit of an edit
    edited = base.edited(moved_scene.hittables)
    base.close()
    assert same_bits(_render_and_gbuffer(edited, cfg), want)
    back = edited.edited(base_scene.hittables)
    edited.close()
    assert same_bits(_render_and_gbuffer(back, cfg), before)
    back.close()


def test_scene_edit_rejects_a_wrong_count():
    s = mixed_scene()
    base = DeviceScene(s)
    out = C.c_void_p(1)
    for n in (s.num_hittables - 1, s.num_hittables + 1, 0):
        assert lib().rt_scene_edit(base.handle, s.hittables, n, C.byref(out)) == -1
        assert b"count" in lib().rt_last_error() and not out.value
    assert lib().rt_scene_edit(base.handle, None, s.num_hittables, C.byref(out)) == -1
    # an invalid description is refused as rt_scene_create refuses it
    bad = mixed_scene()
    bad.hittables[2].radius = -1.0
    assert lib().rt_scene_edit(base.handle, bad.hittables, s.num_hittables, C.byref(out)) == -2 and not out.value
    base.close()


# ---------------------------------------------------------------------------------------------------------------------
# End to end through Renderer
# ---------------------------------------------------------------------------------------------------------------------
def _sequence(cfg, passes: bool):
    """Six frames of the orbit while two spheres are dragged: edited() → render (→ gbuffer → scene_motion → temporal with
    the table).  Returns the renderer and, with the passes, each frame's radiance and G-buffer planes (host copies)."""
    w, h = E2E_SIZE
    r = Renderer(w, h)
    r.render_init()
    ds = DeviceScene(sequence_scene(0))
    frames, gbuffers = [], []
    for k in range(SEQUENCE_FRAMES):
        inp = sequence_inputs(k)
        if k:
            ds, old = ds.edited(sequence_scene(k).hittables), ds
            torch.cuda.synchronize()
            old.close()
        r.render(ds, 1, cfg.depth, inp, radiance=True)
        if passes:
            nd, alb, ids = r.gbuffer(ds, inp, keep_previous=True)
            table = scenes.scene_motion(sequence_scene(k - 1), ds.scene) if k else identity_table(ds.scene.num_hittables)
            r.temporal(prim_motion=table)
            torch.cuda.synchronize()
            frames.append(r.radiance_image().copy())
            gbuffers.append({"normal_depth": nd.cpu().numpy(), "albedo": alb.cpu().numpy(), "prim_id": ids.cpu().numpy()})
    torch.cuda.synchronize()
    ds.close()
    return r, frames, gbuffers


def test_end_to_end_sequence_keeps_history_on_the_moved_objects():
    """C5 at 64x48, 1 spp, depth 4, six frames: against the oracle's 1024-spp radiance of the last scene the GPU pipeline
    satisfies the orderings the numpy pipeline does (table < reset on the whole frame, with and without the filter; table
    < motion ignored on the moved objects' pixels), the other two handlings computed in numpy on the frames and planes
    the GPU rendered.  The render's image and states are the same with and without the passes."""
    cfg = end_to_end_frame()["cfg"]
    r, frames, gbuffers = _sequence(cfg, True)
    r.denoise(source="history")
    torch.cuda.synchronize()
    ref = dynamic_sequence_reference()
    out = numpy_dynamic_sequence(frames, gbuffers)
    want = sequence_errors(out, gbuffers, ref)
    gpu = dict(out, table=r.history.cpu().numpy(), table_filtered=r.denoised.cpu().numpy())
    got = sequence_errors(gpu, gbuffers, ref)
    print("numpy pipeline on the GPU's frames: " + format_errors(want))
    print("GPU pipeline: " + format_errors(got))
    assert_sequence_orderings(want)
    assert_sequence_orderings(got)
    moved = np.isin(gbuffers[-1]["prim_id"], (2, 4))
    assert (gpu["table"][..., 3][moved] >= SEQUENCE_FRAMES - 0.5).any()
    plain, _, _ = _sequence(cfg, False)
    assert np.array_equal(plain.image(), r.image())
    assert np.array_equal(plain.states(), r.states())
    assert plain.radiance.cpu().numpy().tobytes() == r.radiance.cpu().numpy().tobytes()
