"""rt_gbuffer on the GPU against the brute-force reference of tests/test_denoise_host.py (gbuffer_reference), compared
on decidable pixels: those whose centre ray and four rays shifted by +-1/64 pixel hit the same primitive."""
from __future__ import annotations

import ctypes as C

import numpy as np
import pytest
import torch

from cudaraytracer_amd import abi
from cudaraytracer_amd._lib import lib
from cudaraytracer_amd.renderer import DeviceScene, Renderer

from test_denoise_host import UNDECIDABLE_CAP, gbuffer_case

pytestmark = pytest.mark.gpu


def run_gbuffer(ds: DeviceScene, inputs, width: int, height: int, flat_max: int | None = None, **tiling) -> tuple:
    """(normal_depth, albedo, prim_id) of one rt_gbuffer call as numpy arrays, and the renderer's rows."""
    prev = lib().rt_set_tuning(abi.RT_TUNE_FLAT_MAX, flat_max) if flat_max is not None else None
    try:
        r = Renderer(width, height, **tiling)
        nd, alb, prim = r.gbuffer(ds, inputs)
        torch.cuda.synchronize()
        return nd.cpu().numpy(), alb.cpu().numpy(), prim.cpu().numpy(), r.rows
    finally:
        if prev is not None:
            lib().rt_set_tuning(abi.RT_TUNE_FLAT_MAX, prev)


def check_against_reference(name: str, got: tuple) -> None:
    ref = gbuffer_case(name)["ref"]
    nd, alb, prim = got[:3]
    dec = ref["decidable"]
    share = 1.0 - float(dec.mean())
    assert share <= UNDECIDABLE_CAP, share
    wrong = dec & (prim != ref["prim_id"])
    assert not wrong.any(), (int(wrong.sum()), np.argwhere(wrong)[:5], prim[wrong][:5], ref["prim_id"][wrong][:5])
    hit, miss = dec & (ref["prim_id"] >= 0), dec & (ref["prim_id"] < 0)
    t, t_ref = nd[..., 3][hit], ref["normal_depth"][..., 3][hit]
    e_t = float(np.max(np.abs(t - t_ref) / t_ref)) if hit.any() else 0.0
    e_n = float(np.max(np.abs(nd[..., :3][hit] - ref["normal_depth"][..., :3][hit]))) if hit.any() else 0.0
    e_a = float(np.max(np.abs(alb[dec] - ref["albedo"][dec])))
    print(f"{name}: undecidable {share:.4f}, t rel {e_t:.2e}, normal {e_n:.2e}, albedo {e_a:.2e}")
    assert e_t <= 1e-4 and e_n <= 1e-4 and e_a <= 1e-4, (e_t, e_n, e_a)
    assert np.all(alb[..., 3] == 1.0)
    if miss.any():
        assert np.array_equal(nd[miss], np.broadcast_to(np.float32([0, 0, 0, -1]), nd[miss].shape))
        assert np.all(prim[miss] == -1)


@pytest.mark.parametrize("name,flat_max", [("c1", None), ("mixed", None), ("mixed", 0), ("c2", None), ("inactive", None),
                                           ("inactive", 0)])
def test_gbuffer_matches_the_reference(name, flat_max):
    """C1 at 48x32; all three rectangle types, a checker and an image texture at the ragged 50x37; the 488-sphere C2
    scene at 64x40 (BVH path); a description with an inactive hittable in its middle (prim_id counts it).  flat_max 0
    sends a small scene through the BVH path as well (RT_TUNE_FLAT_MAX)."""
    case = gbuffer_case(name)
    ds = DeviceScene(case["scene"])
    check_against_reference(name, run_gbuffer(ds, case["inputs"], case["width"], case["height"], flat_max))


def test_gbuffer_of_a_reference_graph_scene():
    """rt_scene_from_reference_graph: prim_id counts in the order of rt_reference_graph_flatten."""
    case = gbuffer_case("refgraph")
    ds = DeviceScene(reference_graph=C.addressof(case["graph"].world))
    check_against_reference("refgraph", run_gbuffer(ds, case["inputs"], case["width"], case["height"]))


@pytest.mark.parametrize("flat_max", [None, 0])
def test_band_rows_equal_whole_frame_rows(flat_max):
    """rt_tiling: with 2 ranks and band_rows 8 on a 48x40 frame each rank's rows are the whole frame's, bit for bit."""
    case = gbuffer_case("tiling")
    ds = DeviceScene(case["scene"])
    w, h = case["width"], case["height"]
    whole = run_gbuffer(ds, case["inputs"], w, h, flat_max)
    check_against_reference("tiling", whole)
    seen = []
    for rank in (0, 1):
        part = run_gbuffer(ds, case["inputs"], w, h, flat_max, band_rows=8, num_ranks=2, rank=rank)
        rows = part[3]
        seen += rows
        for a, b in zip(part[:3], whole[:3]):
            assert a.tobytes() == b[rows].tobytes()
    assert sorted(seen) == list(range(h))


def test_gbuffer_is_deterministic_and_leaves_the_rng_state_alone():
    case = gbuffer_case("mixed")
    ds = DeviceScene(case["scene"])
    r = Renderer(case["width"], case["height"])
    r.render_init()
    torch.cuda.synchronize()
    before = r.states().copy()
    first = [t.cpu().numpy().copy() for t in r.gbuffer(ds, case["inputs"])]
    torch.cuda.synchronize()
    second = [t.cpu().numpy() for t in r.gbuffer(ds, case["inputs"])]
    for a, b in zip(first, second):
        assert a.tobytes() == b.tobytes()
    assert np.array_equal(r.states(), before)


def test_gbuffer_optional_outputs_and_status_codes():
    """Each plane is optional (a NULL one is not written); a tiling that maps rows outside the image is refused."""
    case = gbuffer_case("c1")
    ds = DeviceScene(case["scene"])
    w, h = case["width"], case["height"]
    full = run_gbuffer(ds, case["inputs"], w, h)
    prim = torch.full((h, w), 77, dtype=torch.int32, device="cuda")
    a = abi.GBufferArgs()
    a.prim_id = prim.data_ptr()
    a.width, a.height = w, h
    a.tiling = abi.Tiling(h, 1, 0, h)
    a.inputs = case["inputs"]
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    assert lib().rt_gbuffer(ds.handle, C.byref(a), stream) == 0
    torch.cuda.synchronize()
    assert np.array_equal(prim.cpu().numpy(), full[2])
    a.tiling = abi.Tiling(h, 2, 1, h)
    assert lib().rt_gbuffer(ds.handle, C.byref(a), stream) == -1
    assert b"tiling" in lib().rt_last_error()
