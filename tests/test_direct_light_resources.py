"""Resource budget of rt_radiance_rays' light-sampling kernel (CPU: reads the gfx950 code objects' metadata, as
test_radiance_resources.py does).

The four builds of radiance_direct_kernel<COUNT_TESTS, WIDE> exist.  The two product builds hold a path's state, the
parked connection term and the parked bounce direction in registers: no scratch (no private segment, no VGPR spills),
no spilled scalar register, no static LDS (the traversal stacks are dynamic LDS sized by the BVH's depth), and the VGPR
counts the build gave, within the 128 of __launch_bounds__(64, 4).  The counting builds carry two
traversals' diagnostic counts and ask for two waves per SIMD; they too stay out of scratch.  The kernel is a template of
its own, and shade()'s new template parameter is defaulted, so every kernel it stands beside — radiance_rays_kernel
among them — keeps the VGPR count the other resource tests pin."""
from test_ray_kernel_resources import DIRECT_VGPRS as PRODUCT_VGPRS  # (the figures: one table)
from test_ray_kernel_resources import _direct
from test_variance_resources import kernel_metadata


def test_direct_light_kernels_use_no_scratch(tmp_path):
    meta = kernel_metadata(tmp_path)
    for count in (0, 1):
        for wide in (0, 1):
            k = _direct(count, wide)
            assert k in meta, k
            print(k, meta[k])
            assert meta[k]["private_segment_fixed_size"] == 0, (k, meta[k])
            assert meta[k]["vgpr_spill_count"] == 0 and meta[k]["sgpr_spill_count"] == 0, (k, meta[k])
            assert meta[k]["group_segment_fixed_size"] == 0, (k, meta[k])
    for k, vgprs in PRODUCT_VGPRS.items():
        assert meta[k]["vgpr_count"] == vgprs, (k, meta[k])
        assert vgprs <= 128
    for wide in (0, 1):  # the counting builds: two waves per SIMD asked for
        assert meta[_direct(1, wide)]["vgpr_count"] <= 256
