"""The per-ray kernels' register pins, in one table (CPU: reads the gfx950 code objects' metadata, as
test_variance_resources.py does).

trace_rays_kernel, radiance_rays_kernel, radiance_direct_kernel, adaptive_samples_kernel and temporal_gradient_kernel
share their wave set-up, schedule and path step (RayWave, ray_wave_run, SampleSums / path_vertex in render.hip), so a
change to a shared piece moves all of them.  query_rays_kernel and occlusion_rays_kernel run the same schedule from
copies of their own (they measured slower on the shared pieces): a change to the schedule has to be made
in those two as well, and their counts move on their own.  The exact VGPR counts of all seven, and those of the kernels
they stand beside, are pinned here and checked by one test.  What is a kernel's own —
no static LDS, no spilled scalar register, a bound on its count, a relation between two kernels — stays in its feature's
file (test_query_resources.py, test_occlusion_resources.py, test_radiance_resources.py, test_direct_light_resources.py,
test_adaptive_resources.py, test_gradient_resources.py), which takes its symbols and figures from this table."""
from test_variance_resources import UNCHANGED_VGPRS as FILTER_VGPRS
from test_variance_resources import kernel_metadata

RAYS_ARGS = "NS0_7KParamsEPK15HIP_vector_typeIfLj4EEjjPS3_IiLj2EE"


def _query(wide):
    return f"_ZN2rt3dev17query_rays_kernelILb{wide}EEEvNS0_11QueryParamsE"


def _gbuffer(flat, wide):
    return f"_ZN2rt3dev14gbuffer_kernelILb{flat}ELb{wide}EEEvNS0_10GBufParamsE"


def _trace(count, wide):
    return f"_ZN2rt3dev17trace_rays_kernelILb{count}ELb{wide}EEEv{RAYS_ARGS}"


def _occlusion(count, wide):
    return f"_ZN2rt3dev21occlusion_rays_kernelILb{count}ELb{wide}EEEvNS0_15OcclusionParamsE"


def _radiance(count, wide):
    return f"_ZN2rt3dev20radiance_rays_kernelILb{count}ELb{wide}EEEvNS0_14RadianceParamsE"


def _direct(count, wide):
    return f"_ZN2rt3dev22radiance_direct_kernelILb{count}ELb{wide}EEEvNS0_20RadianceDirectParamsE"


def _adaptive(count, wide):
    return f"_ZN2rt3dev23adaptive_samples_kernelILb{count}ELb{wide}EEEvNS0_14AdaptiveParamsE"


def _gradient(count, wide):
    return f"_ZN2rt3dev24temporal_gradient_kernelILb{count}ELb{wide}EEEvNS0_14GradientParamsE"


COUNT = "_ZN2rt3dev21adaptive_count_kernelENS0_12SelectParamsE"
WRITE = "_ZN2rt3dev21adaptive_write_kernelENS0_12SelectParamsE"

# VGPRs the build gives, per family.  WIDE builds hold 32-bit stack entries.
# query: 4 waves per SIMD asked for, 6 fit; the WIDE G-buffer and ray-batch builds came with it
NEW_VGPRS = {_query(0): 76, _query(1): 78, _gbuffer(0, 1): 62, _trace(0, 1): 59}
# ... and the 16-bit builds that were there before they were templated on the reference width
UNCHANGED_VGPRS = {_gbuffer(0, 0): 60, _gbuffer(1, 0): 41, _trace(0, 0): 57}
# occlusion, product builds: 4 waves per SIMD asked for, 8 fit
OCCLUSION_VGPRS = {_occlusion(0, 0): 59, _occlusion(0, 1): 61}
# radiance, product builds: 4 waves per SIMD asked for (at most 128), 6 fit.  The counting builds take 118.
RADIANCE_VGPRS = {_radiance(0, 0): 78, _radiance(0, 1): 80}
# direct light, product builds: 4 waves per SIMD asked for (at most 128), 5 fit
DIRECT_VGPRS = {_direct(0, 0): 92, _direct(0, 1): 94}
# adaptive samples and temporal gradient: the counting builds are diagnostics
SAMPLES_VGPRS = {_adaptive(0, 0): 82, _adaptive(0, 1): 84, _adaptive(1, 0): 121, _adaptive(1, 1): 121}
SELECT_VGPRS = {COUNT: 20, WRITE: 23}
GRADIENT_VGPRS = {_gradient(0, 0): 82, _gradient(0, 1): 84, _gradient(1, 0): 120, _gradient(1, 1): 120}

PINNED = {**NEW_VGPRS, **UNCHANGED_VGPRS, **OCCLUSION_VGPRS, **RADIANCE_VGPRS, **DIRECT_VGPRS, **SAMPLES_VGPRS, **SELECT_VGPRS,
          **GRADIENT_VGPRS, **FILTER_VGPRS}


def test_every_pinned_kernel_keeps_its_figures(tmp_path):
    meta = kernel_metadata(tmp_path)
    for k, vgprs in PINNED.items():
        assert k in meta, k
        assert meta[k]["vgpr_count"] == vgprs, (k, meta[k])
        assert meta[k]["private_segment_fixed_size"] == 0, (k, meta[k])
        assert meta[k]["vgpr_spill_count"] == 0, (k, meta[k])
