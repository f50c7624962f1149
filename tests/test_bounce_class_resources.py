"""Resources of the headline v3 builds with the direction-class lookup in v3_bounce_entry (CPU: reads the gfx950 code
object's metadata, the figures of the compiler's resource remarks).

The lookup adds the class of the ray's direction and one multiply-add on the record index to the shading pass; it must
not cost the kernel its 8 waves per SIMD (<= 64 VGPRs), put anything in scratch, or reserve static LDS (the kernel's
LDS is the launch's dynamic allocation).  render_kernel_v3<false, 8, false, PHILOX, true, false>: XORWOW at 62 VGPRs
with no private segment, Philox at 63 with its 12 bytes of cold spill slots, as before the classes.
"""
import os
import re
import shutil
import subprocess

import pytest

from test_kernel_resources import LIB, LLVM, _v3


def _metadata(tmp_path):
    lib = tmp_path / "librt_hip.so"
    shutil.copy(LIB, lib)
    subprocess.run([f"{LLVM}/llvm-objdump", "--offloading", str(lib)], check=True, capture_output=True, cwd=tmp_path)
    co = sorted(f for f in os.listdir(tmp_path) if f.endswith("gfx950"))
    assert co, os.listdir(tmp_path)
    meta = {}
    for c in co:
        notes = subprocess.run([f"{LLVM}/llvm-readelf", "--notes", str(tmp_path / c)], check=True, capture_output=True,
                               text=True).stdout
        # one "- .agpr_count: ..." list item per kernel, its keys in alphabetical order
        for block in re.split(r"\n\s+- \.", notes):
            name = re.search(r"\.name:\s+(\S+)", block)
            if not name:
                continue
            meta[name.group(1)] = {k: int(v) for k, v in re.findall(
                r"\.?(group_segment_fixed_size|private_segment_fixed_size|vgpr_count|vgpr_spill_count):\s+(\d+)", block)}
    return meta


@pytest.mark.skipif(not (os.path.exists(LIB) and os.path.exists(f"{LLVM}/llvm-readelf")), reason="needs the built library and ROCm LLVM tools")
def test_headline_builds_keep_their_registers_scratch_and_lds(tmp_path):
    meta = _metadata(tmp_path)
    xorwow, philox = meta[_v3(0, 0, 1)], meta[_v3(0, 1, 1)]
    for m in (xorwow, philox):
        assert set(m) == {"group_segment_fixed_size", "private_segment_fixed_size", "vgpr_count", "vgpr_spill_count"}, m
        assert m["vgpr_count"] <= 64, m
        assert m["group_segment_fixed_size"] == 0, m
    assert xorwow["private_segment_fixed_size"] == 0 and xorwow["vgpr_spill_count"] == 0, xorwow
    assert philox["private_segment_fixed_size"] <= 12 and philox["vgpr_spill_count"] <= 2, philox
