"""Resource budget of the kernels of rt_temporal_moments and rt_denoise_variance, and the unchanged figures of the kernels
they stand beside (CPU: reads the gfx950 code objects' metadata, as test_kernel_resources.py does).

The new kernels use no scratch and at most 64 KB of LDS (a workgroup's share at which two still fit a compute unit's
160 KB).  temporal_kernel, temporal_dynamic_kernel and every denoise_kernel instantiation keep the VGPR counts they had
before the new kernels existed: the new code is compiled out of them (if constexpr) or lives in templates of its own."""
import os
import re
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "cudaraytracer_amd", "librt_hip.so")
LLVM = "/opt/rocm/lib/llvm/bin"
FIELDS = "name|private_segment_fixed_size|group_segment_fixed_size|vgpr_count|vgpr_spill_count|sgpr_spill_count"

TEMPORAL = "_ZN2rt3dev15temporal_kernelENS_14TemporalParamsE"
TEMPORAL_DYNAMIC = "_ZN2rt3dev23temporal_dynamic_kernelENS_14TemporalParamsEPK15HIP_vector_typeIfLj4EEj"
MOMENTS = "_ZN2rt3dev23temporal_moments_kernelENS_14TemporalParamsEPK15HIP_vector_typeIfLj2EEPS3_"
MOMENTS_DYNAMIC = ("_ZN2rt3dev31temporal_dynamic_moments_kernelENS_14TemporalParamsEPK15HIP_vector_typeIfLj4EEjPKS2_IfLj2EEPS6_")
VARIANCE_STAGE = "_ZN2rt3dev19dnv_variance_kernelENS0_9DnvParamsE"


def _denoise(s, first, last):
    return f"_ZN2rt3dev14denoise_kernelILi{s}ELb{first}ELb{last}EEEvNS0_8DnParamsE"


def _dnv(s, last):
    return f"_ZN2rt3dev10dnv_kernelILi{s}ELb{last}EEEvNS0_9DnvParamsE"


# VGPRs of the kernels the feature must leave alone, as the commit before it compiled them
UNCHANGED_VGPRS = {TEMPORAL: 63, TEMPORAL_DYNAMIC: 63,
                   _denoise(1, 1, 1): 48, _denoise(1, 1, 0): 48, _denoise(2, 0, 1): 41, _denoise(2, 0, 0): 41,
                   _denoise(4, 0, 1): 42, _denoise(4, 0, 0): 42, _denoise(0, 0, 1): 64, _denoise(0, 0, 0): 64}
NEW = [MOMENTS, MOMENTS_DYNAMIC, VARIANCE_STAGE] + [_dnv(s, last) for s in (1, 2, 4, 0) for last in (0, 1)]


def kernel_metadata(tmp_path) -> dict:
    """{kernel name: {field: value}} over every gfx950 code object of the library."""
    lib = tmp_path / "librt_hip.so"
    shutil.copy(LIB, lib)
    subprocess.run([f"{LLVM}/llvm-objdump", "--offloading", str(lib)], check=True, capture_output=True, cwd=tmp_path)
    objects = sorted(f for f in os.listdir(tmp_path) if f.endswith("gfx950"))
    assert objects, os.listdir(tmp_path)
    meta = {}
    for co in objects:
        notes = subprocess.run([f"{LLVM}/llvm-readelf", "--notes", str(tmp_path / co)], check=True, capture_output=True,
                               text=True).stdout
        entry = None
        for line in notes.splitlines():
            if line.startswith("  - ."):  # a kernel's entry begins (its fields come in alphabetical order)
                entry = {}
            m = re.match(rf"\s+(?:- )?\.({FIELDS}):\s+(\S+)", line)
            if not m or entry is None:
                continue
            if m.group(1) == "name":
                meta[m.group(2)] = entry
            else:
                entry[m.group(1)] = int(m.group(2))
    return meta


def test_new_kernels_use_no_scratch_and_fit_the_lds_budget(tmp_path):
    meta = kernel_metadata(tmp_path)
    for k in NEW:
        assert k in meta, k
        print(k, meta[k])
        assert meta[k]["private_segment_fixed_size"] == 0, (k, meta[k])
        assert meta[k]["vgpr_spill_count"] == 0 and meta[k]["sgpr_spill_count"] == 0, (k, meta[k])
        assert meta[k]["group_segment_fixed_size"] <= 64 * 1024, (k, meta[k])
    assert meta[MOMENTS]["group_segment_fixed_size"] == 0 and meta[MOMENTS_DYNAMIC]["group_segment_fixed_size"] == 0
    # the staged tiles: 38×22 pixels of 28 B; 36×20, 40×24 and 48×32 pixels of 32 B; none in the global-memory build
    assert meta[VARIANCE_STAGE]["group_segment_fixed_size"] == 38 * 22 * 28
    for s, tile in ((1, 36 * 20), (2, 40 * 24), (4, 48 * 32), (0, 0)):
        for last in (0, 1):
            assert meta[_dnv(s, last)]["group_segment_fixed_size"] == tile * 32, (s, last)


def test_existing_kernels_keep_their_registers(tmp_path):
    meta = kernel_metadata(tmp_path)
    assert all(k in meta for k in NEW)  # (beside the new kernels: the figures below are what they were without them)
    for k, vgprs in UNCHANGED_VGPRS.items():
        assert k in meta, k
        assert meta[k]["vgpr_count"] == vgprs, (k, meta[k])
        assert meta[k]["private_segment_fixed_size"] == 0, (k, meta[k])
