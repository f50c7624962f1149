"""Resource budget of rt_temporal_gradient's and rt_history_adapt's kernels (CPU: reads the gfx950 code objects' metadata,
as test_adaptive_resources.py does).

The four builds of temporal_gradient_kernel<COUNT_TESTS, WIDE> exist.  They are adaptive_samples_kernel without the
pixel's history and moments in registers, so the product builds need no more VGPRs than that kernel's 86 / 88: no scratch
(no private segment, no VGPR spills), no static LDS (the traversal stacks are dynamic LDS sized by the BVH's depth), and
the VGPR counts the build gave.  history_adapt_kernel is a small stencil: no scratch, no LDS.  The new
kernels are a template and a function of their own, so every kernel they stand beside keeps the VGPR count the other
resource tests pin."""
from test_adaptive_resources import SAMPLES_VGPRS, SELECT_VGPRS, _adaptive
from test_occlusion_resources import PRODUCT_VGPRS as OCCLUSION_VGPRS
from test_query_resources import NEW_VGPRS, UNCHANGED_VGPRS
from test_radiance_resources import PRODUCT_VGPRS as RADIANCE_VGPRS
from test_variance_resources import UNCHANGED_VGPRS as FILTER_VGPRS
from test_variance_resources import kernel_metadata


def _gradient(count, wide):
    return f"_ZN2rt3dev24temporal_gradient_kernelILb{count}ELb{wide}EEEvNS0_14GradientParamsE"


ADAPT = "_ZN2rt3dev20history_adapt_kernelENS0_11AdaptParamsE"
# VGPRs the build gave (4 waves per SIMD asked for: at most 128); the counting builds are diagnostics
GRADIENT_VGPRS = {_gradient(0, 0): 86, _gradient(0, 1): 88, _gradient(1, 0): 124, _gradient(1, 1): 124}
ADAPT_VGPRS = 14


def test_gradient_kernels_use_no_scratch(tmp_path):
    meta = kernel_metadata(tmp_path)
    for k, vgprs in GRADIENT_VGPRS.items():
        assert k in meta, k
        print(k, meta[k])
        assert meta[k]["private_segment_fixed_size"] == 0, (k, meta[k])
        assert meta[k]["vgpr_spill_count"] == 0, (k, meta[k])
        assert meta[k]["group_segment_fixed_size"] == 0, (k, meta[k])
        assert meta[k]["vgpr_count"] == vgprs, (k, meta[k])
        assert vgprs <= 128
    for wide in (0, 1):  # the product builds: nothing spilled at all, and no more registers than adaptive_samples_kernel
        assert meta[_gradient(0, wide)]["sgpr_spill_count"] == 0
        assert GRADIENT_VGPRS[_gradient(0, wide)] <= SAMPLES_VGPRS[_adaptive(0, wide)]
    assert ADAPT in meta
    print(ADAPT, meta[ADAPT])
    assert meta[ADAPT]["private_segment_fixed_size"] == 0 and meta[ADAPT]["group_segment_fixed_size"] == 0, meta[ADAPT]
    assert meta[ADAPT]["vgpr_spill_count"] == 0 and meta[ADAPT]["sgpr_spill_count"] == 0, meta[ADAPT]
    assert meta[ADAPT]["vgpr_count"] == ADAPT_VGPRS, meta[ADAPT]


def test_parent_kernels_keep_their_registers(tmp_path):
    meta = kernel_metadata(tmp_path)
    assert all(k in meta for k in GRADIENT_VGPRS)  # (beside the new kernels: the figures below are what they were without them)
    for k, vgprs in {**NEW_VGPRS, **UNCHANGED_VGPRS, **OCCLUSION_VGPRS, **RADIANCE_VGPRS, **FILTER_VGPRS, **SAMPLES_VGPRS,
                     **SELECT_VGPRS}.items():
        assert k in meta, k
        assert meta[k]["vgpr_count"] == vgprs, (k, meta[k])
        assert meta[k]["private_segment_fixed_size"] == 0, (k, meta[k])
        assert meta[k]["vgpr_spill_count"] == 0, (k, meta[k])
