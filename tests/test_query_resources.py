"""Resource budget of rt_query_rays' kernels and of the 32-bit-reference (WIDE) builds of the G-buffer and ray-batch
kernels (CPU: reads the gfx950 code objects' metadata, as test_variance_resources.py does).

Every new kernel symbol exists, uses no scratch (no private segment, no VGPR spills) and no static LDS (the traversal
stacks are dynamic LDS sized by the BVH's depth), and has the VGPR count the build gave.  The
16-bit-reference builds of gbuffer_kernel and trace_rays_kernel keep the VGPR counts they had before they were
templated on the reference width; the flat G-buffer build, which has no traversal stack, likewise."""
from test_ray_kernel_resources import NEW_VGPRS, UNCHANGED_VGPRS, _query, _trace  # (the figures: one table)
from test_variance_resources import kernel_metadata


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
