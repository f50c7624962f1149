"""Resource budget of rt_query_rays' kernels and of the 32-bit-reference (WIDE) builds of the G-buffer and ray-batch
kernels (CPU: reads the gfx950 code objects' metadata, as test_variance_resources.py does).

Every new kernel symbol exists, uses no scratch (no private segment, no VGPR spills) and no static LDS (the traversal
stacks are dynamic LDS sized by the BVH's depth), and has the VGPR count the build gave.  The
16-bit-reference builds of gbuffer_kernel and trace_rays_kernel keep the VGPR counts they had before they were
templated on the reference width; the flat G-buffer build, which has no traversal stack, likewise."""
from test_variance_resources import kernel_metadata

RAYS_ARGS = "NS0_7KParamsEPK15HIP_vector_typeIfLj4EEjjPS3_IiLj2EE"


def _query(wide):
    return f"_ZN2rt3dev17query_rays_kernelILb{wide}EEEvNS0_11QueryParamsE"


def _gbuffer(flat, wide):
    return f"_ZN2rt3dev14gbuffer_kernelILb{flat}ELb{wide}EEEvNS0_10GBufParamsE"


def _trace(count, wide):
    return f"_ZN2rt3dev17trace_rays_kernelILb{count}ELb{wide}EEEv{RAYS_ARGS}"


# VGPRs the build gave the new kernels (query: 4 waves per SIMD asked for, 6 fit; the WIDE builds hold 32-bit entries)
NEW_VGPRS = {_query(0): 76, _query(1): 78, _gbuffer(0, 1): 62, _trace(0, 1): 60}
# ... and those of the 16-bit builds before this feature (gbuffer_kernel<FLAT>, trace_rays_kernel<COUNT_TESTS = false>)
UNCHANGED_VGPRS = {_gbuffer(0, 0): 60, _gbuffer(1, 0): 41, _trace(0, 0): 58}


def test_new_kernels_use_no_scratch(tmp_path):
    meta = kernel_metadata(tmp_path)
    for k, vgprs in NEW_VGPRS.items():
        assert k in meta, k
        print(k, meta[k])
        assert meta[k]["private_segment_fixed_size"] == 0, (k, meta[k])
        assert meta[k]["vgpr_spill_count"] == 0, (k, meta[k])
        assert meta[k]["group_segment_fixed_size"] == 0, (k, meta[k])
        assert meta[k]["vgpr_count"] == vgprs, (k, meta[k])
    # the query kernels hold up to four of their 106 SGPRs in VGPR lanes (v_writelane / v_readlane): registers, no memory
    for wide in (0, 1):
        assert meta[_query(wide)]["sgpr_spill_count"] <= 4, meta[_query(wide)]
    # the counting build of the ray-batch kernel (a diagnostic, tools/coherence.py) exists for both widths
    assert _trace(1, 0) in meta and _trace(1, 1) in meta


def test_sixteen_bit_builds_keep_their_registers(tmp_path):
    meta = kernel_metadata(tmp_path)
    for k, vgprs in UNCHANGED_VGPRS.items():
        assert k in meta, k
        assert meta[k]["vgpr_count"] == vgprs, (k, meta[k])
        assert meta[k]["private_segment_fixed_size"] == 0, (k, meta[k])
        assert meta[k]["vgpr_spill_count"] == 0 and meta[k]["sgpr_spill_count"] == 0, (k, meta[k])
