"""Resource budget of rt_adaptive_samples' and rt_adaptive_select's kernels (CPU: reads the gfx950 code objects' metadata,
as test_radiance_resources.py does).

The four builds of adaptive_samples_kernel<COUNT_TESTS, WIDE> exist.  They hold a path's state, the pixel's history and
moments and the entry's sums in registers: no scratch (no private segment, no VGPR spills), no static LDS (the traversal
stacks are dynamic LDS sized by the BVH's depth), and the VGPR counts the build gave: the product builds
take 4 more than radiance_rays_kernel's and, at most 96, still fit five waves per SIMD.  The two selection kernels are
small: no scratch, 16 bytes of LDS (one word per wave of the workgroup).  The new kernels are templates and functions of
their own, so every kernel they stand beside keeps the VGPR count the other resource tests pin."""
from test_occlusion_resources import PRODUCT_VGPRS as OCCLUSION_VGPRS
from test_query_resources import NEW_VGPRS, UNCHANGED_VGPRS
from test_radiance_resources import PRODUCT_VGPRS as RADIANCE_VGPRS
from test_variance_resources import UNCHANGED_VGPRS as FILTER_VGPRS
from test_variance_resources import kernel_metadata


def _adaptive(count, wide):
    return f"_ZN2rt3dev23adaptive_samples_kernelILb{count}ELb{wide}EEEvNS0_14AdaptiveParamsE"


COUNT = "_ZN2rt3dev21adaptive_count_kernelENS0_12SelectParamsE"
WRITE = "_ZN2rt3dev21adaptive_write_kernelENS0_12SelectParamsE"
# VGPRs the build gave (4 waves per SIMD asked for: at most 128); the counting builds are diagnostics
SAMPLES_VGPRS = {_adaptive(0, 0): 86, _adaptive(0, 1): 88, _adaptive(1, 0): 125, _adaptive(1, 1): 125}
SELECT_VGPRS = {COUNT: 20, WRITE: 23}


def test_adaptive_kernels_use_no_scratch(tmp_path):
    meta = kernel_metadata(tmp_path)
    for k, vgprs in SAMPLES_VGPRS.items():
        assert k in meta, k
        print(k, meta[k])
        assert meta[k]["private_segment_fixed_size"] == 0, (k, meta[k])
        assert meta[k]["vgpr_spill_count"] == 0, (k, meta[k])
        assert meta[k]["group_segment_fixed_size"] == 0, (k, meta[k])
        assert meta[k]["vgpr_count"] == vgprs, (k, meta[k])
        assert vgprs <= 128
    for wide in (0, 1):  # the product builds: nothing spilled at all, and five waves per SIMD
        assert meta[_adaptive(0, wide)]["sgpr_spill_count"] == 0
        assert SAMPLES_VGPRS[_adaptive(0, wide)] <= 96
    for k, vgprs in SELECT_VGPRS.items():
        assert k in meta, k
        print(k, meta[k])
        assert meta[k]["private_segment_fixed_size"] == 0 and meta[k]["group_segment_fixed_size"] == 16, (k, meta[k])
        assert meta[k]["vgpr_spill_count"] == 0 and meta[k]["sgpr_spill_count"] == 0, (k, meta[k])
        assert meta[k]["vgpr_count"] == vgprs, (k, meta[k])


def test_parent_kernels_keep_their_registers(tmp_path):
    meta = kernel_metadata(tmp_path)
    assert all(k in meta for k in SAMPLES_VGPRS)  # (beside the new kernels: the figures below are what they were without them)
    for k, vgprs in {**NEW_VGPRS, **UNCHANGED_VGPRS, **OCCLUSION_VGPRS, **RADIANCE_VGPRS, **FILTER_VGPRS}.items():
        assert k in meta, k
        assert meta[k]["vgpr_count"] == vgprs, (k, meta[k])
        assert meta[k]["private_segment_fixed_size"] == 0, (k, meta[k])
        assert meta[k]["vgpr_spill_count"] == 0, (k, meta[k])
