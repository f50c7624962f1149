"""Resource budget of rt_adaptive_samples' and rt_adaptive_select's kernels (CPU: reads the gfx950 code objects' metadata,
as test_radiance_resources.py does).

The four builds of adaptive_samples_kernel<COUNT_TESTS, WIDE> exist.  They hold a path's state, the pixel's history and
moments and the entry's sums in registers: no scratch (no private segment, no VGPR spills), no static LDS (the traversal
stacks are dynamic LDS sized by the BVH's depth), and the VGPR counts the build gave: the product builds
take 4 more than radiance_rays_kernel's and, at most 96, still fit five waves per SIMD.  The two selection kernels are
small: no scratch, 16 bytes of LDS (one word per wave of the workgroup).  The new kernels are templates and functions of
their own, so every kernel they stand beside keeps the VGPR count the other resource tests pin."""
from test_ray_kernel_resources import SAMPLES_VGPRS, SELECT_VGPRS, _adaptive  # (the figures: one table)
from test_variance_resources import kernel_metadata


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
