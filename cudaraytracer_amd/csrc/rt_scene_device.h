// rt_scene_device.h — the opaque rt_scene handle: host copy of the packed tables + device pointers.
#pragma once

#include <cstdint>
#include <memory>

#include "rt_internal.h"

namespace rt {

struct DeviceScene {
    const void* nodes = nullptr;   // float4 × 4 per node
    const void* nodes48 = nullptr; // float4 × 3 per node (boxes only)
    const void* refs = nullptr;    // per node: uint32 of two 16-bit child references, or (wide_refs) two uint32
    bool wide_refs = false;
    const void* prims = nullptr;   // float4 × 2 per primitive
    const void* prims_flat = nullptr;  // the same records in the reference BVH's test order (small scenes), or NULL
    const void* ref_nodes = nullptr;   // the reference BVH (boxes + shape) over prims_flat, or NULL
    const void* flat_ref_pairs = nullptr;  // ... as child-pair records (the flat kernels' wave-serial replay)
    const void* flat_boxes = nullptr;  // per prims_flat record its reference box (exactness check), or NULL
    const void* bvh_ref_nodes = nullptr;  // the reference BVH over `prims` (BVH order), or NULL (bvh_clear, render.hip)
    const void* bvh_boxes = nullptr;      // per `prims` record its reference box, or NULL
    const void* bvh_ref_pairs = nullptr;  // per reference node its children's boxes and references (ref_trace_wave)
    uint32_t flat_runs[2] = {0u, 0u};  // HostScene::flat_runs
    const void* prim_source = nullptr;  // per `prims` record the index of its hittable in the caller's description
    const void* flat_source = nullptr;  // ... per prims_flat record, or NULL (rt_gbuffer's prim_id)
    const void* leaf_records = nullptr;  // bounce entries (rt_bounce_entry.h): uint4 per leaf, or NULL = no table
    const void* bounce_grid = nullptr;   // ... uint16 per grid cell: the index of a leaf record
    const void* class_records = nullptr; // ... uint4 per (leaf record, direction class), or NULL (rt_set_bounce_classes)
    uint32_t grid_dim[3] = {0u, 0u, 0u};
    float grid_inv[3] = {0.0f, 0.0f, 0.0f}, grid_off[3] = {0.0f, 0.0f, 0.0f};
    const void* light_table = nullptr;  // HostScene::light_table (NULL without a rectangle); num_rects and num_lights
    uint32_t num_rects = 0, num_lights = 0;  // ... say where its per-primitive words begin and how many lights it lists
    const void* mats = nullptr;    // float4 × 3 per material
    const void* imgs = nullptr;    // int4 per image
    const void* texels = nullptr;  // RGB8
    uint32_t num_nodes = 0, num_prims = 0, num_mats = 0, depth = 0;
    uint32_t num_imgs = 0;  // image descriptors (int4 each)
    bool has_image_textures = false;
    bool has_textures = false;  // any CHECKER or IMAGE albedo (selects the texture-capable kernel)
    bool has_rects = false;     // HostScene::has_rects
    uint64_t device_bytes = 0;
    uint64_t uid = 0;  // unique per created device scene (a handle's address can be reused; render.hip EntryTable)
};

// Upload the tables of `h` to the current device.  shared_texels: an existing device texel block (same image
// table) to reference instead of uploading h.texels.  The host copy of the texels is not kept.
int create_device_scene(const HostScene& h, rt_scene** out, std::shared_ptr<void> shared_texels = nullptr);

// The device scene of the reference graph `world` for LaunchKernel (Kernel.cu:178-191), cached per
// (device, world): materials edited in place are re-uploaded, geometry edits rebuild the BVH and tables but
// keep the uploaded texels, a new image (data pointer, width or height, CudaLayer.cpp:889-903) re-uploads
// them.  *host_ms: host time spent (flatten + compare + any update).
int reference_scene_for_launch(const void* world, std::shared_ptr<rt_scene>* out, double* host_ms);

}  // namespace rt

struct rt_scene {
    rt::HostScene host;  // packed tables (texels dropped after the upload)
    rt::DeviceScene dev;
    std::shared_ptr<void> texel_block;  // device texels, shared by scenes rebuilt from the same images
    // The part of the description rt_scene_edit needs (rt_scene_create keeps it; LaunchKernel's cached scenes do not:
    // described = false).  images[i].data is NULL or a placeholder for "has texels": the host texels are not kept.
    bool described = false;
    uint32_t num_hittables = 0;  // entries of the caller's hittable list, inactive ones counted
    std::vector<rt_material_desc> materials;  // as the last rt_scene_update_materials left them
    std::vector<rt_image_desc> images;
    int texel_bytes = 3;            // device bytes per texel of texel_block (RT_TUNE_TEXEL_LAYOUT when it was uploaded)
    uint64_t texel_block_bytes = 0; // size of texel_block
};
