"""Resource budget of the kernels the automatic choice runs (CPU: reads the gfx950 code object's metadata).

A private array that LLVM materialises in scratch (it happened to the Philox word select: scratch loads on
every draw, +8 % frame time) or a register count past 64 (8 waves per SIMD) is a performance regression
the parity tests cannot see.  This test pins "no scratch" for the v3 (variants 2, 3) and v4 (variant 4)
kernels in both RNG modes, with and without texture support, and <= 72 VGPRs for the v3 kernels of
untextured scenes (<= 64 for the XORWOW and Philox builds of variant 3, the headline kernels; the texture-capable and persistent kernels run at 85-98
VGPRs, 5 waves per SIMD, measured in DESIGN.md)."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "cudaraytracer_amd", "librt_hip.so")
LLVM = "/opt/rocm/lib/llvm/bin"

# render_kernel_v3<COUNT_TESTS=false, W, TEX, PHILOX, COMPACT, WIDE> (variants 2 and 3; the untextured compact
# 16-bit-reference builds are held to 8 waves per SIMD by registers (both RNG modes), render.hip
# k*CompactWaves; the 32-bit-reference (WIDE) builds exist for the compact v3 and v4 only)
# render_kernel_v4<COUNT_TESTS=false, TEX, NODES_64=2, PHILOX, WIDE, WAVES_PER_SIMD=1, TRACE> (variant 4; TRACE = 1 is
# the wave-trace build picked only while rt_set_wave_trace holds a buffer)
def _v3(t, p, c, wd=0):
    w = 8 if (c and not t and not wd) else 1
    return f"_ZN2rt3dev16render_kernel_v3ILb0ELi{w}ELb{t}ELb{p}ELb{c}ELb{wd}EEEvNS0_7KParamsE"


def _v4(t, p, wd=0, trace=0):
    return f"_ZN2rt3dev16render_kernel_v4ILb0ELb{t}ELi2ELb{p}ELb{wd}ELi1ELb{trace}EEEvNS0_7KParamsE"


HOT = [_v3(t, p, c) for t in (0, 1) for p in (0, 1) for c in (0, 1)] + [_v4(t, p) for t in (0, 1) for p in (0, 1)] + \
      [_v3(t, p, 1, 1) for t in (0, 1) for p in (0, 1)] + [_v4(t, p, 1) for t in (0, 1) for p in (0, 1)]
# register-held builds: a few bytes of cold spills (measured faster than the compiler's register count)
# (the Philox build reserves 36 B of stack for SGPR spill slots its code never touches: no scratch instruction; since
# round 6 the XORWOW v4 builds likewise: their code holds no scratch instruction).  No v3/v4 build calls a function any more (the reference replay of
# bvh_clear runs inline, ref_trace_wave), so none reserves a callee's frame.
SPILL_OK = {_v3(0, 0, 1): 32, _v3(0, 1, 1): 48, _v4(1, 0): 36, _v4(1, 0, 1): 36, _v4(0, 0): 36}


def kernel_metadata(tmp_path):
    lib = tmp_path / "librt_hip.so"
    shutil.copy(LIB, lib)
    subprocess.run([f"{LLVM}/llvm-objdump", "--offloading", str(lib)], check=True, capture_output=True, cwd=tmp_path)
    # one code object per .hip file: all of them (the directory's listing order differs between file systems, and the
    # first entry is render.hip's on some only)
    co = sorted(f for f in os.listdir(tmp_path) if f.endswith("gfx950"))
    assert co, os.listdir(tmp_path)
    notes = "\n".join(subprocess.run([f"{LLVM}/llvm-readelf", "--notes", str(tmp_path / c)], check=True,
                                     capture_output=True, text=True).stdout for c in co)
    meta, name = {}, None
    for line in notes.splitlines():
        m = re.match(r"\s+\.(name|private_segment_fixed_size|vgpr_count|vgpr_spill_count|sgpr_spill_count):\s+(\S+)", line)
        if not m:
            continue
        if m.group(1) == "name":
            name = m.group(2)
            meta[name] = {}
        elif name is not None:
            meta[name][m.group(1)] = int(m.group(2))
    return meta


@pytest.mark.skipif(not (os.path.exists(LIB) and os.path.exists(f"{LLVM}/llvm-readelf")), reason="needs the built library and ROCm LLVM tools")
def test_hot_kernels_register_and_scratch_budget(tmp_path):
    meta = kernel_metadata(tmp_path)
    for k in HOT:
        assert k in meta, k
        assert meta[k]["private_segment_fixed_size"] <= SPILL_OK.get(k, 0), (k, meta[k])
        if "render_kernel_v3ILb0ELi1ELb0ELb0E" in k or k == _v3(0, 0, 1):  # untextured XORWOW builds
            assert meta[k]["vgpr_count"] <= 72, (k, meta[k])
    # the default kernel of untextured many-sample frames (variant 3, XORWOW) at 8 waves per SIMD
    assert meta[_v3(0, 0, 1)]["vgpr_count"] <= 64
    assert meta[_v3(0, 1, 1)]["vgpr_count"] <= 64


def _flat(t, p, persistent=False, trace=0, group=2):
    if persistent:  # (GROUP 2: 16-wave workgroups drawing chunks, the default; 1: static shares; 0: round 5's one-wave form)
        return f"_ZN2rt3dev29render_kernel_flat_persistentILb0ELb{t}ELb{p}ELi1ELb{trace}ELi{group}EEEvNS0_7KParamsE"
    return f"_ZN2rt3dev18render_kernel_flatILb0ELb{t}ELb{p}ELi{8 if not t else 1}EEEvNS0_7KParamsE"


@pytest.mark.skipif(not (os.path.exists(LIB) and os.path.exists(f"{LLVM}/llvm-readelf")), reason="needs the built library and ROCm LLVM tools")
def test_flat_kernels_register_and_scratch_budget(tmp_path):
    """The flat kernels (variants 5, 6): the untextured tile build at 8 waves per SIMD (<= 64 VGPRs), and a private
    segment no larger than the reference replay's frame (ref_trace: its 16-entry stack, touched only by the rare rays
    that replay the reference BVH) plus a few bytes of cold spills."""
    meta = kernel_metadata(tmp_path)
    for t in (0, 1):
        for p in (0, 1):
            for k in (_flat(t, p), _flat(t, p, True), _flat(t, p, True, group=1), _flat(t, p, True, group=0)):
                assert k in meta, k
                assert meta[k]["private_segment_fixed_size"] <= 192, (k, meta[k])
    assert meta[_flat(0, 0)]["vgpr_count"] <= 64
    assert meta[_flat(0, 1)]["vgpr_count"] <= 64
    # the persistent kernels' wave-trace builds exist beside the product builds, which carry none of the trace's
    # registers: the textured XORWOW persistent flat kernel (C5) spilled 105 SGPRs to VGPR lanes with the run-time
    # checked trace, 26 now (profiles/r05q_ab_c5_trace_build.txt)
    for t in (0, 1):
        for p in (0, 1):
            assert _flat(t, p, True, trace=1) in meta and _v4(t, p, trace=1) in meta
    assert meta[_flat(1, 0, True, group=0)]["sgpr_spill_count"] <= 40, meta[_flat(1, 0, True, group=0)]
    # round 6: the GROUP builds (2, the default: chunk queue; 1: static shares) each carry only their own scheduling
    # code, and the wave id is read as an SGPR (readfirstlane) — computed per lane it had put the queue's head index in
    # VGPRs: 82 spills, 504 v_readlane
    assert meta[_flat(1, 0, True)]["sgpr_spill_count"] <= 32, meta[_flat(1, 0, True)]
    assert meta[_flat(1, 0, True, group=1)]["sgpr_spill_count"] <= 72, meta[_flat(1, 0, True, group=1)]  # (a knob, not the default)
