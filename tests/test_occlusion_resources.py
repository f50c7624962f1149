"""Resource budget of rt_occluded_rays' kernels (CPU: reads the gfx950 code objects' metadata, as
test_variance_resources.py does).

The four builds of occlusion_rays_kernel<COUNT_TESTS, WIDE> exist; the two product builds (COUNT_TESTS = false) use no
scratch (no private segment, no VGPR spills), no static LDS (the traversal stacks are dynamic LDS sized by the BVH's
depth), keep no more SGPRs in VGPR lanes than query_rays_kernel does, and have the VGPR counts the build gave
(DESIGN.md §16).  The any-hit mode is a template parameter of v3_traverse whose default leaves every other
instantiation as it was: query_rays_kernel, trace_rays_kernel<false, *> and gbuffer_kernel keep the VGPR counts
tests/test_ray_kernel_resources.py pins (one table and one test for every per-ray kernel)."""
from test_ray_kernel_resources import OCCLUSION_VGPRS as PRODUCT_VGPRS  # (the figures: one table)
from test_ray_kernel_resources import _occlusion, _query
from test_variance_resources import kernel_metadata


def test_occlusion_kernels_use_no_scratch(tmp_path):
    meta = kernel_metadata(tmp_path)
    for count in (0, 1):
        for wide in (0, 1):
            assert _occlusion(count, wide) in meta, (count, wide)
    query_lanes = max(meta[_query(w)]["sgpr_spill_count"] for w in (0, 1))
    for k, vgprs in PRODUCT_VGPRS.items():
        print(k, meta[k])
        assert meta[k]["private_segment_fixed_size"] == 0, (k, meta[k])
        assert meta[k]["vgpr_spill_count"] == 0, (k, meta[k])
        assert meta[k]["group_segment_fixed_size"] == 0, (k, meta[k])
        assert meta[k]["sgpr_spill_count"] <= query_lanes, (k, meta[k])
        assert meta[k]["vgpr_count"] == vgprs, (k, meta[k])
    # the counting builds are diagnostics; they too stay out of scratch
    for wide in (0, 1):
        assert meta[_occlusion(1, wide)]["private_segment_fixed_size"] == 0
        assert meta[_occlusion(1, wide)]["group_segment_fixed_size"] == 0
