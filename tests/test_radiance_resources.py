"""Resource budget of rt_radiance_rays' and rt_camera_rays' kernels (CPU: reads the gfx950 code objects' metadata, as
test_occlusion_resources.py does).

The four builds of radiance_rays_kernel<COUNT_TESTS, WIDE> and camera_rays_kernel exist.  The two product builds
(COUNT_TESTS = false) keep a whole path's state in registers: no scratch (no private segment, no VGPR spills), no
static LDS (the traversal stacks are dynamic LDS sized by the BVH's depth), and the VGPR counts the build gave
(DESIGN.md §17), which stay within the 128 of __launch_bounds__(64, 4).  The kernels are templates of their own that
call v3_traverse, shade and camera_ray as they are, so every kernel they stand beside keeps the VGPR count that
tests/test_ray_kernel_resources.py pins (one table and one test for every per-ray kernel)."""
from test_ray_kernel_resources import RADIANCE_VGPRS as PRODUCT_VGPRS  # (the figures: one table)
from test_ray_kernel_resources import _radiance
from test_variance_resources import kernel_metadata

CAMERA = "_ZN2rt3dev18camera_rays_kernelENS0_16CameraRaysParamsE"


def test_radiance_kernels_use_no_scratch(tmp_path):
    meta = kernel_metadata(tmp_path)
    for count in (0, 1):
        for wide in (0, 1):
            assert _radiance(count, wide) in meta, (count, wide)
    assert CAMERA in meta
    for k, vgprs in PRODUCT_VGPRS.items():
        print(k, meta[k])
        assert meta[k]["private_segment_fixed_size"] == 0, (k, meta[k])
        assert meta[k]["vgpr_spill_count"] == 0, (k, meta[k])
        assert meta[k]["group_segment_fixed_size"] == 0, (k, meta[k])
        assert meta[k]["vgpr_count"] == vgprs, (k, meta[k])
        assert vgprs <= 128
    # the counting builds are diagnostics; they too stay out of scratch
    for wide in (0, 1):
        assert meta[_radiance(1, wide)]["private_segment_fixed_size"] == 0
        assert meta[_radiance(1, wide)]["group_segment_fixed_size"] == 0
    print(CAMERA, meta[CAMERA])
    assert meta[CAMERA]["private_segment_fixed_size"] == 0 and meta[CAMERA]["group_segment_fixed_size"] == 0
    assert meta[CAMERA]["vgpr_spill_count"] == 0 and meta[CAMERA]["sgpr_spill_count"] == 0
