"""Resource budget of the direct-light builds of the two fused frame passes (CPU: reads the gfx950 code objects' metadata,
as test_direct_light_resources.py does).

adaptive_direct_kernel<COUNT_TESTS, WIDE> and gradient_direct_kernel<COUNT_TESTS, WIDE> — rt_adaptive_samples and
rt_temporal_gradient with RT_RADIANCE_DIRECT_LIGHT — exist in all eight builds.  Each holds its sibling's state plus the
shadow state (the parked term, the parked bounce direction, the path's direct sum) in registers: no scratch (no private
segment, no VGPR spill), no spilled scalar register, no static LDS beyond the flagless sibling's (none: the traversal
stacks are dynamic LDS).  The product builds have the VGPR counts the build gave, within the 128 of
__launch_bounds__(64, 4); the counting builds carry two traversals' diagnostic counts and ask for two waves per SIMD.
The kernels are templates of their own beside the flagless ones, whose pins test_ray_kernel_resources.py keeps."""
from test_ray_kernel_resources import _adaptive, _gradient
from test_variance_resources import kernel_metadata


def _adaptive_direct(count, wide):
    return f"_ZN2rt3dev22adaptive_direct_kernelILb{count}ELb{wide}EEEvNS0_20AdaptiveDirectParamsE"


def _gradient_direct(count, wide):
    return f"_ZN2rt3dev22gradient_direct_kernelILb{count}ELb{wide}EEEvNS0_20GradientDirectParamsE"


# product builds: 4 waves per SIMD asked for; 5 fit at 96 or fewer
PRODUCT_VGPRS = {_adaptive_direct(0, 0): 96, _adaptive_direct(0, 1): 100, _gradient_direct(0, 0): 93, _gradient_direct(0, 1): 95}
SIBLING = {_adaptive_direct: _adaptive, _gradient_direct: _gradient}


def test_direct_frame_kernels_use_no_scratch(tmp_path):
    meta = kernel_metadata(tmp_path)
    for family, sibling in SIBLING.items():
        for count in (0, 1):
            for wide in (0, 1):
                k = family(count, wide)
                assert k in meta, k
                print(k, meta[k])
                assert meta[k]["private_segment_fixed_size"] == 0, (k, meta[k])
                assert meta[k]["vgpr_spill_count"] == 0 and meta[k]["sgpr_spill_count"] == 0, (k, meta[k])
                assert meta[k]["group_segment_fixed_size"] <= meta[sibling(count, wide)]["group_segment_fixed_size"], (k, meta[k])
                assert meta[k]["vgpr_count"] <= (256 if count else 128), (k, meta[k])  # two and four waves per SIMD
    for k, vgprs in PRODUCT_VGPRS.items():
        assert meta[k]["vgpr_count"] == vgprs, (k, meta[k])
        assert vgprs <= 128
