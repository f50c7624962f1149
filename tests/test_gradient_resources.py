"""Resource budget of rt_temporal_gradient's and rt_history_adapt's kernels (CPU: reads the gfx950 code objects' metadata,
as test_adaptive_resources.py does).

The four builds of temporal_gradient_kernel<COUNT_TESTS, WIDE> exist.  They are adaptive_samples_kernel without the
pixel's history and moments in registers, so the product builds need no more VGPRs than that kernel's 82 / 84: no scratch
(no private segment, no VGPR spills), no static LDS (the traversal stacks are dynamic LDS sized by the BVH's depth), and
the VGPR counts the build gave.  history_adapt_kernel is a small stencil: no scratch, no LDS.  The new
kernels are a template and a function of their own, so every kernel they stand beside keeps the VGPR count the other
resource tests pin."""
from test_ray_kernel_resources import GRADIENT_VGPRS, SAMPLES_VGPRS, _adaptive, _gradient  # (the figures: one table)
from test_variance_resources import kernel_metadata

ADAPT = "_ZN2rt3dev20history_adapt_kernelENS0_11AdaptParamsE"
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
