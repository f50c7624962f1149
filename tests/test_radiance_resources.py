"""Resource budget of rt_radiance_rays' and rt_camera_rays' kernels (CPU: reads the gfx950 code objects' metadata, as
test_occlusion_resources.py does).

The four builds of radiance_rays_kernel<COUNT_TESTS, WIDE> and camera_rays_kernel exist.  The two product builds
(COUNT_TESTS = false) keep a whole path's state in registers: no scratch (no private segment, no VGPR spills), no
static LDS (the traversal stacks are dynamic LDS sized by the BVH's depth), and the VGPR counts the build gave
(DESIGN.md §17), which stay within the 128 of __launch_bounds__(64, 4).  The kernels are templates of their own that
call v3_traverse, shade and camera_ray as they are, so every kernel they stand beside keeps the VGPR count that
tests/test_query_resources.py and tests/test_occlusion_resources.py pin."""
from test_occlusion_resources import PRODUCT_VGPRS as OCCLUSION_VGPRS
from test_query_resources import NEW_VGPRS, UNCHANGED_VGPRS
from test_variance_resources import kernel_metadata


def _radiance(count, wide):
    return f"_ZN2rt3dev20radiance_rays_kernelILb{count}ELb{wide}EEEvNS0_14RadianceParamsE"


CAMERA = "_ZN2rt3dev18camera_rays_kernelENS0_16CameraRaysParamsE"
# VGPRs the build gave the product kernels (4 waves per SIMD asked for: at most 128; 5 fit; the WIDE build holds 32-bit
# entries).  The counting builds take 122 and no scratch either.
PRODUCT_VGPRS = {_radiance(0, 0): 82, _radiance(0, 1): 84}


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


def test_ray_batch_kernels_keep_their_registers(tmp_path):
    meta = kernel_metadata(tmp_path)
    assert all(k in meta for k in PRODUCT_VGPRS)  # (beside the new kernels: the figures below are what they were without them)
    for k, vgprs in {**NEW_VGPRS, **UNCHANGED_VGPRS, **OCCLUSION_VGPRS}.items():
        assert k in meta, k
        assert meta[k]["vgpr_count"] == vgprs, (k, meta[k])
        assert meta[k]["private_segment_fixed_size"] == 0, (k, meta[k])
        assert meta[k]["vgpr_spill_count"] == 0, (k, meta[k])
