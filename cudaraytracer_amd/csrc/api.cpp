// api.cpp — host half of the C ABI: error reporting, device scene tables, and the flattener for the
// reference's pointer-graph scene (the `Hittable* world` argument of LaunchKernel, Kernel.cu:178-180).
#include <hip/hip_runtime_api.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <cmath>
#include <new>
#include <stdexcept>
#include <cstring>
#include <mutex>
#include <unordered_set>

#include "../../include/rt_reference_graph.h"
#include "rt_bounce_entry.h"
#include "rt_internal.h"
#include "rt_scene_device.h"

namespace rt {

static thread_local std::string g_last_error;

void set_error(const std::string& msg) { g_last_error = msg; }

// Host steps allocate (std::vector, std::string): a failed allocation must come back as a status code, not
// as an exception through the extern "C" boundary (which would terminate the caller's process).
template <class F>
static int guarded(const char* what, F&& f) {
    try {
        return f();
    } catch (const std::bad_alloc&) {
        set_error(std::string(what) + ": host allocation failed");
        return RT_ERR_OUT_OF_MEMORY;
    } catch (const std::exception& e) {
        set_error(std::string(what) + ": " + e.what());
        return RT_ERR_INVALID_SCENE;
    }
}

static int hip_fail(hipError_t e, const char* what) {
    set_error(std::string(what) + ": " + hipGetErrorString(e));
    return e == hipErrorOutOfMemory ? RT_ERR_OUT_OF_MEMORY : RT_ERR_DEVICE;
}

template <typename T>
static int upload(const std::vector<T>& host, void** dev, const char* what) {
    *dev = nullptr;
    if (host.empty()) return RT_OK;
    hipError_t e = hipMalloc(dev, host.size() * sizeof(T));
    if (e != hipSuccess) return hip_fail(e, what);
    e = hipMemcpy(*dev, host.data(), host.size() * sizeof(T), hipMemcpyHostToDevice);
    if (e != hipSuccess) {
        (void)hipFree(*dev);
        *dev = nullptr;
        return hip_fail(e, what);
    }
    return RT_OK;
}

static void free_device(DeviceScene* s) {
    if (s->nodes) (void)hipFree((void*)s->nodes);
    if (s->nodes48) (void)hipFree((void*)s->nodes48);
    if (s->refs) (void)hipFree((void*)s->refs);
    s->nodes48 = s->refs = nullptr;
    if (s->prims) (void)hipFree((void*)s->prims);
    if (s->prims_flat) (void)hipFree((void*)s->prims_flat);
    if (s->ref_nodes) (void)hipFree((void*)s->ref_nodes);
    if (s->flat_boxes) (void)hipFree((void*)s->flat_boxes);
    if (s->flat_ref_pairs) (void)hipFree((void*)s->flat_ref_pairs);
    s->prims_flat = s->ref_nodes = s->flat_boxes = s->flat_ref_pairs = nullptr;
    if (s->bvh_ref_nodes) (void)hipFree((void*)s->bvh_ref_nodes);
    if (s->bvh_boxes) (void)hipFree((void*)s->bvh_boxes);
    if (s->bvh_ref_pairs) (void)hipFree((void*)s->bvh_ref_pairs);
    s->bvh_ref_nodes = s->bvh_boxes = s->bvh_ref_pairs = nullptr;
    if (s->leaf_records) (void)hipFree((void*)s->leaf_records);
    if (s->bounce_grid) (void)hipFree((void*)s->bounce_grid);
    if (s->class_records) (void)hipFree((void*)s->class_records);
    s->leaf_records = s->bounce_grid = s->class_records = nullptr;
    if (s->prim_source) (void)hipFree((void*)s->prim_source);
    if (s->flat_source) (void)hipFree((void*)s->flat_source);
    s->prim_source = s->flat_source = nullptr;
    if (s->light_table) (void)hipFree((void*)s->light_table);
    s->light_table = nullptr;
    if (s->mats) (void)hipFree((void*)s->mats);
    if (s->imgs) (void)hipFree((void*)s->imgs);  // texels: owned by rt_scene::texel_block
    s->nodes = s->prims = s->mats = nullptr;
    s->imgs = nullptr;
    s->texels = nullptr;
}

int create_device_scene(const HostScene& h, rt_scene** out, std::shared_ptr<void> shared_texels) {
    rt_scene* s = new rt_scene();
    s->host = h;
    s->host.texels = std::vector<uint8_t>();  // uploaded below (or shared); no host copy is kept
    DeviceScene& d = s->dev;
    static std::atomic<uint64_t> next_uid{1};
    d.uid = next_uid.fetch_add(1);
    int rc;
    void* p;
    if ((rc = upload(h.nodes, &p, "hipMalloc/hipMemcpy(nodes)"))) goto fail;
    d.nodes = p;
    if ((rc = upload(h.nodes48, &p, "hipMalloc/hipMemcpy(nodes48)"))) goto fail;
    d.nodes48 = p;
    if ((rc = upload(h.refs, &p, "hipMalloc/hipMemcpy(refs)"))) goto fail;
    d.refs = p;
    d.wide_refs = h.wide_refs;
    if ((rc = upload(h.prims, &p, "hipMalloc/hipMemcpy(prims)"))) goto fail;
    d.prims = p;
    if ((rc = upload(h.prims_flat, &p, "hipMalloc/hipMemcpy(prims_flat)"))) goto fail;
    d.prims_flat = p;
    if ((rc = upload(h.ref_nodes, &p, "hipMalloc/hipMemcpy(ref_nodes)"))) goto fail;
    d.ref_nodes = p;
    if ((rc = upload(h.flat_ref_pairs, &p, "hipMalloc/hipMemcpy(flat_ref_pairs)"))) goto fail;
    d.flat_ref_pairs = p;
    if ((rc = upload(h.flat_boxes, &p, "hipMalloc/hipMemcpy(flat_boxes)"))) goto fail;
    d.flat_boxes = p;
    if ((rc = upload(h.bvh_ref_nodes, &p, "hipMalloc/hipMemcpy(bvh_ref_nodes)"))) goto fail;
    d.bvh_ref_nodes = p;
    if ((rc = upload(h.bvh_boxes, &p, "hipMalloc/hipMemcpy(bvh_boxes)"))) goto fail;
    d.bvh_boxes = p;
    if ((rc = upload(h.bvh_ref_pairs, &p, "hipMalloc/hipMemcpy(bvh_ref_pairs)"))) goto fail;
    d.bvh_ref_pairs = p;
    d.flat_runs[0] = h.flat_runs[0];
    d.flat_runs[1] = h.flat_runs[1];
    if (!h.bounce_grid.empty()) {
        if ((rc = upload(h.leaf_records, &p, "hipMalloc/hipMemcpy(leaf_records)"))) goto fail;
        d.leaf_records = p;
        if ((rc = upload(h.bounce_grid, &p, "hipMalloc/hipMemcpy(bounce_grid)"))) goto fail;
        d.bounce_grid = p;
        if ((rc = upload(h.class_records, &p, "hipMalloc/hipMemcpy(class_records)"))) goto fail;
        d.class_records = p;
        for (int i = 0; i < 3; i++) {
            d.grid_dim[i] = h.grid_dim[i];
            d.grid_inv[i] = h.grid_inv[i];
            d.grid_off[i] = h.grid_off[i];
        }
    }
    if ((rc = upload(h.prim_source, &p, "hipMalloc/hipMemcpy(prim_source)"))) goto fail;
    d.prim_source = p;
    if ((rc = upload(h.flat_source, &p, "hipMalloc/hipMemcpy(flat_source)"))) goto fail;
    d.flat_source = p;
    if ((rc = upload(h.light_table, &p, "hipMalloc/hipMemcpy(light_table)"))) goto fail;
    d.light_table = p;
    d.num_rects = (uint32_t)(h.rects.size() / 8);
    d.num_lights = (uint32_t)h.lights.size();
    if ((rc = upload(h.mats, &p, "hipMalloc/hipMemcpy(materials)"))) goto fail;
    d.mats = p;
    if ((rc = upload(h.imgs, &p, "hipMalloc/hipMemcpy(images)"))) goto fail;
    d.imgs = p;
    if (shared_texels) {
        s->texel_block = std::move(shared_texels);
    } else {
        if ((rc = upload(h.texels, &p, "hipMalloc/hipMemcpy(texels)"))) goto fail;
        if (p) s->texel_block = std::shared_ptr<void>(p, [](void* q) { (void)hipFree(q); });
    }
    d.texels = s->texel_block.get();
    d.num_nodes = h.num_nodes;
    d.num_prims = h.num_prims;
    d.num_mats = h.num_mats;
    d.num_imgs = (uint32_t)(h.imgs.size() / 4);
    d.depth = h.depth;
    d.has_image_textures = h.has_image_textures;
    d.has_textures = h.has_textures;
    d.has_rects = h.has_rects;
    d.device_bytes = (h.nodes.size() + h.nodes48.size() + h.refs.size() + h.prims.size() + h.prims_flat.size() + h.ref_nodes.size() +
                      h.flat_boxes.size() + h.flat_ref_pairs.size() + h.bvh_ref_nodes.size() + h.bvh_boxes.size() + h.bvh_ref_pairs.size() + h.mats.size() +
                      h.prim_source.size() + h.flat_source.size() + h.leaf_records.size() + h.class_records.size() + h.light_table.size()) * 4 + h.bounce_grid.size() * 2 +
                     h.imgs.size() * 4 + h.texels.size();
    *out = s;
    return RT_OK;
fail:
    free_device(&d);
    delete s;
    return rc;
}

// What rt_scene_edit rebuilds a scene from: the materials, the images' sizes (and whether each had data: the texels
// themselves stay on the device) and the hittable count that gives rt_gbuffer's prim_id values their meaning.
// A failed host allocation frees the new scene, clears the handle and goes on to the caller's guard.
static void keep_description(rt_scene** scene, const rt_scene_desc& d, int texel_bytes) {
    static const uint8_t kHasData = 0;  // stands for "this image has texels"; never read (build_host_scene, with_texels = false)
    rt_scene* s = *scene;
    try {
        s->materials.assign(d.materials, d.materials + d.num_materials);
        s->images.assign(d.images, d.images + d.num_images);
    } catch (...) {
        rt_scene_destroy(s);
        *scene = nullptr;
        throw;
    }
    for (rt_image_desc& im : s->images)
        if (im.data) im.data = &kHasData;
    s->num_hittables = d.num_hittables;
    s->texel_bytes = texel_bytes;
    s->described = true;
}

// ------------------------------------------------------------------------------------------------
// Reference pointer-graph flattener.  Walks BVHNode::left/right (Hittable.cuh:296-301) from `world`,
// collects each distinct leaf hittable once (span-1 leaves reference one object twice, Hittable.cuh:
// 326-327), and resolves Material → {Lambertian|Metal|Dielectric|DiffuseLight} → Texture →
// {Constant|Checker|Image} (Material.cuh:19-177, Texture.cuh:16-109).  The graph only contains active
// objects (the BVH is rebuilt without inactive ones), so every collected hittable is active.
// ------------------------------------------------------------------------------------------------
static int read_texture(const void* tex_ptr, rt_texture_desc* t, FlatDesc* out, std::string* err) {
    std::memset(t, 0, sizeof(*t));
    t->image = -1;
    if (!tex_ptr) { *err = "material without texture"; return RT_ERR_INVALID_SCENE; }
    const rtref_texture* tex = (const rtref_texture*)tex_ptr;
    t->type = tex->type;
    if (!tex->object || !*tex->object) { *err = "texture without object"; return RT_ERR_INVALID_SCENE; }
    const void* obj = *tex->object;
    switch (tex->type) {
    case RT_CONSTANT: {
        const rtref_constant* c = (const rtref_constant*)obj;
        std::memcpy(t->color, c->color.e, sizeof(t->color));
        break;
    }
    case RT_CHECKER: {
        const rtref_checker* c = (const rtref_checker*)obj;
        if (!c->odd || !c->even) { *err = "checker without constants"; return RT_ERR_INVALID_SCENE; }
        std::memcpy(t->color, c->odd->color.e, sizeof(t->color));
        std::memcpy(t->color2, c->even->color.e, sizeof(t->color2));
        break;
    }
    case RT_IMAGE: {
        const rtref_image* im = (const rtref_image*)obj;
        rt_image_desc d;
        d.data = im->data;
        d.width = im->data ? im->width : 0;
        d.height = im->data ? im->height : 0;
        t->image = (int32_t)out->images.size();
        out->images.push_back(d);
        break;
    }
    default: *err = "unknown texture type " + std::to_string(tex->type); return RT_ERR_INVALID_SCENE;
    }
    return RT_OK;
}

static int read_material(const void* mat_ptr, rt_material_desc* m, FlatDesc* out, std::string* err) {
    std::memset(m, 0, sizeof(*m));
    m->albedo.image = -1;
    if (!mat_ptr) { *err = "hittable without material"; return RT_ERR_INVALID_SCENE; }
    const rtref_material* mat = (const rtref_material*)mat_ptr;
    if (!mat->object || !*mat->object) { *err = "material without object"; return RT_ERR_INVALID_SCENE; }
    const void* obj = *mat->object;
    m->type = mat->type;
    switch (mat->type) {
    case RT_LAMBERTIAN: return read_texture(((const rtref_lambertian*)obj)->albedo, &m->albedo, out, err);
    case RT_METAL:
        m->fuzz = ((const rtref_metal*)obj)->fuzz;
        return read_texture(((const rtref_metal*)obj)->albedo, &m->albedo, out, err);
    case RT_DIELECTRIC: m->ir = ((const rtref_dielectric*)obj)->ir; return RT_OK;
    case RT_DIFFUSELIGHT:
        m->light_intensity = ((const rtref_diffuse_light*)obj)->light_intensity;
        return read_texture(((const rtref_diffuse_light*)obj)->albedo, &m->albedo, out, err);
    default: *err = "unknown material type " + std::to_string(mat->type); return RT_ERR_INVALID_SCENE;
    }
}

int flatten_reference_graph(const void* world, FlatDesc* out, std::string* err) {
    *out = FlatDesc();
    if (!world) { *err = "world is NULL"; return RT_ERR_INVALID_ARGUMENT; }
    const rtref_hittable* root = (const rtref_hittable*)world;
    if (root->type != RTREF_BVHNODE) { *err = "world is not a BVHNode hittable"; return RT_ERR_INVALID_SCENE; }
    std::vector<const rtref_hittable*> stack{root};
    std::unordered_set<const void*> seen_nodes, seen_prims;
    while (!stack.empty()) {
        const rtref_hittable* h = stack.back();
        stack.pop_back();
        if (!h->object || !*h->object) { *err = "hittable without object"; return RT_ERR_INVALID_SCENE; }
        const void* obj = *h->object;
        if (h->type == RTREF_BVHNODE) {
            if (!seen_nodes.insert(obj).second) continue;
            if (seen_nodes.size() > (1u << 24)) { *err = "BVH graph too large or cyclic"; return RT_ERR_INVALID_SCENE; }
            const rtref_bvh_node* n = (const rtref_bvh_node*)obj;
            // right first so that the left subtree is emitted first (list order of the build)
            if (n->right) stack.push_back(n->right);
            if (n->left) stack.push_back(n->left);
            continue;
        }
        if (!seen_prims.insert(obj).second) continue;
        rt_hittable_desc d;
        std::memset(&d, 0, sizeof(d));
        d.type = h->type;
        d.is_active = 1;
        const void* mat_ptr;
        if (h->type == RTREF_SPHERE) {
            const rtref_sphere* s = (const rtref_sphere*)obj;
            std::memcpy(d.center, s->center.e, sizeof(d.center));
            d.radius = s->radius;
            mat_ptr = s->mat_ptr;
        } else if (h->type == RTREF_XYRECT || h->type == RTREF_XZRECT || h->type == RTREF_YZRECT) {
            const rtref_rect* r = (const rtref_rect*)obj;
            std::memcpy(d.center, r->center.e, sizeof(d.center));
            d.width = r->width;
            d.height = r->height;
            mat_ptr = r->mat_ptr;
        } else {
            *err = "unsupported hittable type " + std::to_string(h->type) + " in BVH";
            return RT_ERR_INVALID_SCENE;
        }
        rt_material_desc m;
        int rc = read_material(mat_ptr, &m, out, err);
        if (rc) return rc;
        d.material = (int32_t)out->materials.size();
        out->materials.push_back(m);
        out->hittables.push_back(d);
    }
    return RT_OK;
}

// ------------------------------------------------------------------------------------------------
// LaunchKernel's scene cache.  The viewer mutates its managed-memory graph in place
// between frames without notifying anyone, so every launch re-flattens it (microseconds for ~500
// objects) and compares the flat description with the cached one:
//   * hittables (geometry, activity) differ → rebuild BVH + tables, keep the uploaded texels;
//   * only materials differ → re-upload the material table in place (no rebuild, CudaLayer.cpp:719-872);
//   * an image's (data pointer, width, height) differs → rebuild with a new texel upload.  The reference
//     replaces texture data by cudaFree + a new allocation (CudaLayer.cpp:889-903), so the pointer is the
//     change key: texel bytes are never read per frame.
// One entry per (device, world pointer), least recently used evicted beyond kLaunchCacheEntries.
// ------------------------------------------------------------------------------------------------
namespace {

struct ImageKey {
    const void* data;
    int32_t width, height;
    bool operator==(const ImageKey& o) const { return data == o.data && width == o.width && height == o.height; }
};

struct LaunchEntry {
    int device = 0;
    const void* world = nullptr;
    uint64_t last_use = 0;
    std::vector<rt_hittable_desc> hittables;
    std::vector<rt_material_desc> materials;
    std::vector<ImageKey> images;
    int texel_bytes = 0;  // device bytes per texel of the uploaded block (RT_TUNE_TEXEL_LAYOUT when it was made)
    int bounce_classes = 0;  // rt_set_bounce_classes when the tables were built
    // shared with the LaunchKernel calls rendering it: an entry evicted or rebuilt by another thread frees
    // its device scene only when the last of them has finished
    std::shared_ptr<rt_scene> scene;
};

std::shared_ptr<rt_scene> own_scene(rt_scene* s, int device) {
    return std::shared_ptr<rt_scene>(s, [device](rt_scene* p) {
        int cur = 0;
        const bool restore = hipGetDevice(&cur) == hipSuccess;
        (void)hipSetDevice(device);
        rt_scene_destroy(p);
        if (restore) (void)hipSetDevice(cur);
    });
}

constexpr size_t kLaunchCacheEntries = 8;
std::mutex g_launch_mu;
// never destroyed: the entries free device memory, which must not run after the HIP runtime has shut down
std::vector<LaunchEntry>& g_launch_cache = *new std::vector<LaunchEntry>();
uint64_t g_launch_clock = 0;

template <class T>
bool same_bytes(const std::vector<T>& a, const std::vector<T>& b) {
    return a.size() == b.size() && (a.empty() || std::memcmp(a.data(), b.data(), a.size() * sizeof(T)) == 0);
}

}  // namespace

int reference_scene_for_launch(const void* world, std::shared_ptr<rt_scene>* out, double* host_ms) {
    const auto t0 = std::chrono::steady_clock::now();
    int device = 0;
    hipError_t e = hipGetDevice(&device);
    if (e != hipSuccess) return hip_fail(e, "LaunchKernel: hipGetDevice");
    std::lock_guard<std::mutex> lock(g_launch_mu);
    int rc = guarded("LaunchKernel", [&]() -> int {
        FlatDesc f;
        std::string err;
        int r = flatten_reference_graph(world, &f, &err);
        if (r) { set_error("LaunchKernel: " + err); return r; }
        std::vector<ImageKey> images;
        for (const rt_image_desc& im : f.images) images.push_back(ImageKey{im.data, im.width, im.height});
        LaunchEntry* ent = nullptr;
        for (LaunchEntry& c : g_launch_cache)
            if (c.device == device && c.world == world) ent = &c;
        if (!ent) {
            if (g_launch_cache.size() >= kLaunchCacheEntries) {  // evict the least recently used entry
                auto lru = std::min_element(g_launch_cache.begin(), g_launch_cache.end(),
                                            [](const LaunchEntry& a, const LaunchEntry& b) { return a.last_use < b.last_use; });
                g_launch_cache.erase(lru);  // (its scene is freed once no call renders it)
            }
            g_launch_cache.emplace_back();
            ent = &g_launch_cache.back();
            ent->device = device;
            ent->world = world;
        }
        ent->last_use = ++g_launch_clock;
        const bool geometry = !ent->scene || !same_bytes(ent->hittables, f.hittables) ||
                              ent->materials.size() != f.materials.size() || ent->bounce_classes != g_bounce_classes;
        // the image table of a rebuilt scene takes this thread's texel layout: a block uploaded in the other
        // layout cannot be shared with it (its offsets and strides differ), so a layout change re-uploads
        const int texel_bytes = g_texel_bytes == 4 ? 4 : 3;
        const bool new_images = !ent->scene || !(ent->images == images) || ent->texel_bytes != texel_bytes;
        if (geometry || new_images) {
            rt_scene_desc d = f.desc();
            HostScene h;
            r = build_host_scene(&d, &h, &err, new_images);
            if (r) { set_error("LaunchKernel: " + err); return r; }
            rt_scene* fresh = nullptr;
            r = create_device_scene(h, &fresh, new_images ? nullptr : ent->scene->texel_block);
            if (r) return r;
            ent->scene = own_scene(fresh, device);
            ent->texel_bytes = texel_bytes;
            ent->bounce_classes = g_bounce_classes;
        } else if (!same_bytes(ent->materials, f.materials)) {
            r = rt_scene_update_materials(ent->scene.get(), f.materials.data(), (uint32_t)f.materials.size());
            if (r) return r;
        }
        ent->hittables.swap(f.hittables);
        ent->materials.swap(f.materials);
        ent->images.swap(images);
        *out = ent->scene;
        return RT_OK;
    });
    if (host_ms) *host_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    return rc;
}

}  // namespace rt

using namespace rt;

extern "C" {

const char* rt_last_error(void) { return g_last_error.c_str(); }

const char* rt_version(void) { return "librt_hip 0.1 (gfx950)"; }
int rt_abi_version(void) { return RT_ABI_VERSION; }

int rt_set_device(int device) {
    hipError_t e = hipSetDevice(device);
    if (e != hipSuccess) return hip_fail(e, "hipSetDevice");
    return RT_OK;
}

int rt_scene_create(const rt_scene_desc* desc, rt_scene** out_scene) {
    if (!out_scene) { set_error("rt_scene_create: out_scene is NULL"); return RT_ERR_INVALID_ARGUMENT; }
    *out_scene = nullptr;
    return guarded("rt_scene_create", [&]() -> int {
        HostScene h;
        std::string err;
        int rc = build_host_scene(desc, &h, &err);
        if (rc) { set_error("rt_scene_create: " + err); return rc; }
        rc = create_device_scene(h, out_scene);
        if (rc) return rc;
        keep_description(out_scene, *desc, g_texel_bytes == 4 ? 4 : 3);
        (*out_scene)->texel_block_bytes = h.texels.size();
        return RT_OK;
    });
}

int rt_scene_from_reference_graph(const void* world, rt_scene** out_scene) {
    if (!out_scene) { set_error("rt_scene_from_reference_graph: out_scene is NULL"); return RT_ERR_INVALID_ARGUMENT; }
    *out_scene = nullptr;
    return guarded("rt_scene_from_reference_graph", [&]() -> int {
        FlatDesc f;
        std::string err;
        int rc = flatten_reference_graph(world, &f, &err);
        if (rc) { set_error("rt_scene_from_reference_graph: " + err); return rc; }
        rt_scene_desc d = f.desc();
        return rt_scene_create(&d, out_scene);
    });
}

int rt_scene_update_materials(rt_scene* scene, const rt_material_desc* materials, uint32_t num_materials) {
    if (!scene || (!materials && num_materials)) {
        set_error("rt_scene_update_materials: NULL argument");
        return RT_ERR_INVALID_ARGUMENT;
    }
    if (num_materials != scene->dev.num_mats) {
        set_error("rt_scene_update_materials: material count differs from the scene's");
        return RT_ERR_INVALID_ARGUMENT;
    }
    return guarded("rt_scene_update_materials", [&]() -> int {
        std::vector<float> packed;
        std::string err;
        int rc = pack_materials(materials, num_materials, (uint32_t)(scene->host.imgs.size() / 4), &packed, &err);
        if (rc) { set_error("rt_scene_update_materials: " + err); return rc; }
        bool img = false, tex = false;
        for (uint32_t i = 0; i < num_materials; i++) {
            if (materials[i].type == RT_DIELECTRIC) continue;
            img |= materials[i].albedo.type == RT_IMAGE;
            tex |= materials[i].albedo.type != RT_CONSTANT;
        }
        if (!packed.empty()) {
            // renders are asynchronous on the callers' streams: let every launch that may still read the
            // old table finish before it is overwritten (the viewer edits between frames, CudaLayer.cpp:719-872)
            hipError_t e = hipDeviceSynchronize();
            if (e != hipSuccess) return hip_fail(e, "rt_scene_update_materials: hipDeviceSynchronize");
            e = hipMemcpy((void*)scene->dev.mats, packed.data(), packed.size() * 4, hipMemcpyHostToDevice);
            if (e != hipSuccess) return hip_fail(e, "rt_scene_update_materials: hipMemcpy");
        }
        scene->dev.has_image_textures = img;
        scene->dev.has_textures = tex;
        scene->host.mats = packed;
        // a material edit can turn a rectangle into a sampled light or back: the list again, uploaded in place (the
        // table holds an entry for every rectangle whatever the materials are)
        build_light_table(&scene->host);
        if (!scene->host.light_table.empty()) {
            hipError_t e = hipMemcpy((void*)scene->dev.light_table, scene->host.light_table.data(),
                                     scene->host.light_table.size() * 4, hipMemcpyHostToDevice);
            if (e != hipSuccess) return hip_fail(e, "rt_scene_update_materials: hipMemcpy(light_table)");
        }
        scene->dev.num_lights = (uint32_t)scene->host.lights.size();
        if (scene->described) scene->materials.assign(materials, materials + num_materials);  // what rt_scene_edit rebuilds from
        return RT_OK;
    });
}

int rt_reference_graph_flatten(const void* world, rt_hittable_desc* hittables, uint32_t* num_hittables,
                               rt_material_desc* materials, uint32_t* num_materials, rt_image_desc* images,
                               uint32_t* num_images) {
    if (!num_hittables || !num_materials || !num_images) {
        set_error("rt_reference_graph_flatten: count pointers must not be NULL");
        return RT_ERR_INVALID_ARGUMENT;
    }
    FlatDesc f;
    int rc = guarded("rt_reference_graph_flatten", [&]() -> int {
        std::string err;
        int r = flatten_reference_graph(world, &f, &err);
        if (r) set_error("rt_reference_graph_flatten: " + err);
        return r;
    });
    if (rc) return rc;
    bool fits = (!hittables || f.hittables.size() <= *num_hittables) &&
                (!materials || f.materials.size() <= *num_materials) && (!images || f.images.size() <= *num_images);
    if (fits) {
        if (hittables) std::copy(f.hittables.begin(), f.hittables.end(), hittables);
        if (materials) std::copy(f.materials.begin(), f.materials.end(), materials);
        if (images) std::copy(f.images.begin(), f.images.end(), images);
    }
    *num_hittables = (uint32_t)f.hittables.size();
    *num_materials = (uint32_t)f.materials.size();
    *num_images = (uint32_t)f.images.size();
    if (!fits) { set_error("rt_reference_graph_flatten: output arrays too small"); return RT_ERR_INVALID_ARGUMENT; }
    return RT_OK;
}

int rt_build_host_tables(const rt_scene_desc* desc, float* nodes, float* prims, float* materials,
                         int32_t* prim_source, rt_host_tables_info* info) {
    if (!info) { set_error("rt_build_host_tables: info is NULL"); return RT_ERR_INVALID_ARGUMENT; }
    HostScene h;
    int rc = guarded("rt_build_host_tables", [&]() -> int {
        std::string err;
        int r = build_host_scene(desc, &h, &err);
        if (r) set_error("rt_build_host_tables: " + err);
        return r;
    });
    if (rc) return rc;
    info->num_nodes = h.num_nodes;
    info->num_prims = h.num_prims;
    info->num_materials = h.num_mats;
    info->depth = h.depth;
    if (nodes) std::copy(h.nodes.begin(), h.nodes.begin() + (size_t)h.num_nodes * 16, nodes);
    // (num_prims records: an empty scene's table carries one zero record for the device, not for the caller)
    if (prims) std::copy(h.prims.begin(), h.prims.begin() + (size_t)h.num_prims * 8, prims);
    if (materials) std::copy(h.mats.begin(), h.mats.end(), materials);
    if (prim_source) std::copy(h.prim_source.begin(), h.prim_source.end(), prim_source);
    return RT_OK;
}

int rt_scene_lights_host(const rt_scene_desc* desc, uint32_t* hittables, uint32_t capacity, uint32_t* count) {
    if (!count || (!hittables && capacity)) {
        set_error("rt_scene_lights_host: NULL count, or NULL hittables with a capacity");
        return RT_ERR_INVALID_ARGUMENT;
    }
    HostScene h;
    int rc = guarded("rt_scene_lights_host", [&]() -> int {
        std::string err;
        int r = build_host_scene(desc, &h, &err, false);
        if (r) set_error("rt_scene_lights_host: " + err);
        return r;
    });
    if (rc) return rc;
    *count = (uint32_t)h.lights.size();
    std::copy(h.lights.begin(), h.lights.begin() + std::min<size_t>(h.lights.size(), capacity), hittables);
    return RT_OK;
}

int rt_bounce_entries_host(const rt_scene_desc* desc, float* chain_nodes, float* nodes48, uint32_t* refs,
                           uint32_t* records, uint16_t* grid, rt_bounce_entries_info* info) {
    if (!info) { set_error("rt_bounce_entries_host: info is NULL"); return RT_ERR_INVALID_ARGUMENT; }
    HostScene h;
    int rc = guarded("rt_bounce_entries_host", [&]() -> int {
        std::string err;
        int r = build_host_scene(desc, &h, &err);
        if (r) set_error("rt_bounce_entries_host: " + err);
        return r;
    });
    if (rc) return rc;
    std::memset(info, 0, sizeof(*info));
    info->num_nodes = h.num_nodes;
    info->depth = h.depth;
    if (h.bounce_grid.empty()) return RT_OK;  // no table: num_records = 0
    info->num_chain_nodes = h.num_chain_nodes;
    info->num_records = (uint32_t)(h.leaf_records.size() / 4);
    for (int i = 0; i < 3; i++) {
        info->grid_dim[i] = h.grid_dim[i];
        info->grid_origin[i] = h.grid_origin[i];
        info->grid_inv[i] = h.grid_inv[i];
        info->grid_off[i] = h.grid_off[i];
    }
    if (chain_nodes) std::copy(h.chain_nodes.begin(), h.chain_nodes.end(), chain_nodes);
    // (the direction classes' nodes, behind these, are rt_bounce_class_entries_host's)
    const size_t total = (size_t)h.num_nodes + h.num_chain_nodes;
    if (nodes48) std::copy(h.nodes48.begin(), h.nodes48.begin() + total * 12, nodes48);
    if (refs) std::copy(h.refs.begin(), h.refs.begin() + total, refs);
    if (records) std::copy(h.leaf_records.begin(), h.leaf_records.end(), records);
    if (grid) std::copy(h.bounce_grid.begin(), h.bounce_grid.end(), grid);
    return RT_OK;
}

int rt_bounce_entry_cells(const rt_bounce_entries_info* info, const float* origins, uint32_t n, uint32_t* cells) {
    if (!info || (n && (!origins || !cells))) { set_error("rt_bounce_entry_cells: NULL argument"); return RT_ERR_INVALID_ARGUMENT; }
    if (info->num_records == 0 || !info->grid_dim[0] || !info->grid_dim[1] || !info->grid_dim[2]) {
        set_error("rt_bounce_entry_cells: the scene has no bounce-entry table");
        return RT_ERR_INVALID_ARGUMENT;
    }
    const float dimf[3] = {(float)(info->grid_dim[0] - 1u), (float)(info->grid_dim[1] - 1u), (float)(info->grid_dim[2] - 1u)};
    for (uint32_t i = 0; i < n; i++)
        cells[i] = bounce_cell(origins[3 * (size_t)i], origins[3 * (size_t)i + 1], origins[3 * (size_t)i + 2], info->grid_inv,
                               info->grid_off, dimf, info->grid_dim);
    return RT_OK;
}

int rt_set_bounce_classes(int form) {
    if (form < 0 || form > 2) {
        set_error("rt_set_bounce_classes: the value must be 0, 1 or 2");
        return RT_ERR_INVALID_ARGUMENT;
    }
    const int prev = g_bounce_classes;
    g_bounce_classes = form;
    return prev;
}

int rt_bounce_class_entries_host(const rt_scene_desc* desc, int form, uint32_t node_limit, uint32_t* records,
                                 float* class_nodes48, uint32_t* class_refs, double* regions, const float* origins,
                                 const float* directions, uint32_t n, uint32_t* classes, rt_bounce_class_info* info) {
    if (!info) { set_error("rt_bounce_class_entries_host: info is NULL"); return RT_ERR_INVALID_ARGUMENT; }
    if (form < -1 || form > 2) { set_error("rt_bounce_class_entries_host: form must be -1, 0, 1 or 2"); return RT_ERR_INVALID_ARGUMENT; }
    if (node_limit > 0x7fffu) { set_error("rt_bounce_class_entries_host: node_limit must be at most 0x7fff"); return RT_ERR_INVALID_ARGUMENT; }
    if (n && (!directions || !classes)) { set_error("rt_bounce_class_entries_host: NULL directions or classes"); return RT_ERR_INVALID_ARGUMENT; }
    HostScene h;
    const int prev_form = g_bounce_classes;
    const uint32_t prev_limit = g_bounce_class_node_limit;
    if (form >= 0) g_bounce_classes = form;
    if (node_limit) g_bounce_class_node_limit = node_limit;
    int rc = guarded("rt_bounce_class_entries_host", [&]() -> int {
        std::string err;
        int r = build_host_scene(desc, &h, &err);
        if (r) set_error("rt_bounce_class_entries_host: " + err);
        return r;
    });
    g_bounce_classes = prev_form;
    g_bounce_class_node_limit = prev_limit;
    if (rc) return rc;
    std::memset(info, 0, sizeof(*info));
    info->num_records = (uint32_t)(h.leaf_records.size() / 4);
    info->form = h.bounce_classes;
    info->num_class_nodes = h.num_class_nodes;
    info->first_class_node = h.num_nodes + h.num_chain_nodes;
    if (h.bounce_classes) {
        if (records) std::copy(h.class_records.begin(), h.class_records.end(), records);
        const size_t first = info->first_class_node;
        if (class_nodes48) std::copy(h.nodes48.begin() + first * 12, h.nodes48.end(), class_nodes48);
        if (class_refs) std::copy(h.refs.begin() + first, h.refs.end(), class_refs);
        if (regions) std::copy(h.class_regions.begin(), h.class_regions.end(), regions);
    }
    if (n) {
        if (h.bounce_grid.empty()) {
            set_error("rt_bounce_class_entries_host: the scene has no bounce-entry table");
            return RT_ERR_INVALID_ARGUMENT;
        }
        const float dims[3] = {(float)h.grid_dim[0], (float)h.grid_dim[1], (float)h.grid_dim[2]};
        const float zero[3] = {0.0f, 0.0f, 0.0f};
        for (uint32_t i = 0; i < n; i++)
            classes[i] = origins ? bounce_class_at(origins + 3 * (size_t)i, directions + 3 * (size_t)i, h.grid_inv, h.grid_off, dims)
                                 : bounce_class(directions[3 * (size_t)i], directions[3 * (size_t)i + 1],
                                                directions[3 * (size_t)i + 2], zero[0], zero[1], zero[2]);
    }
    return RT_OK;
}

// A camera's launch-uniform terms (Kernel.cu:130-143; the library is compiled with -ffp-contract=off, so every
// operation below is one binary32 rounding, as in render.hip's fill_camera).
static TemporalCamera temporal_camera(const rt_input_struct& in) {
    TemporalCamera c;
    const float* up = in.up;
    const float* fw = in.orientation;
    // rightV = Normalize(Cross(upV, forwardV)) (Kernel.cu:133, Math.cuh:157-161, 225-229)
    const float cx = up[1] * fw[2] - up[2] * fw[1];
    const float cy = -(up[0] * fw[2] - up[2] * fw[0]);
    const float cz = up[0] * fw[1] - up[1] * fw[0];
    const float inv = 1.0f / std::sqrt((cx * cx + cy * cy) + cz * cz);
    c.right[0] = inv * cx;
    c.right[1] = inv * cy;
    c.right[2] = inv * cz;
    c.fov = in.fov;
    c.k10 = (1.0f / in.fov) * 10.0f;
    c.near_plane = in.near_plane;
    c.far_plane = in.far_plane;
    for (int i = 0; i < 3; i++) {
        c.origin[i] = in.origin[i];
        c.fw[i] = fw[i];
        c.up[i] = up[i];
        c.fov_fwd[i] = in.fov * fw[i];
        c.k10_fwd[i] = c.k10 * fw[i];
    }
    c.fw_dot_fw = (fw[0] * fw[0] + fw[1] * fw[1]) + fw[2] * fw[2];
    return c;
}

// The checks of rt_temporal (and, under its own name, of rt_temporal_dynamic) and the launch parameters: RT_OK with *P
// filled and *pixels = width · height, or RT_ERR_INVALID_ARGUMENT with the error set.  No device call.
static int temporal_params(const char* who, const rt_temporal_args* a, TemporalParams* out, uint64_t* pixels) {
    const auto bad = [who](const char* msg) {
        set_error(std::string(who) + ": " + msg);
        return (int)RT_ERR_INVALID_ARGUMENT;
    };
    if (!a) return bad("NULL args");
    if (a->reserved[0] != 0 || a->reserved[1] != 0) return bad("reserved fields must be 0");
    if (a->flags & ~(uint32_t)(RT_TEMPORAL_COLOR_IS_SUM | RT_TEMPORAL_RESET)) return bad("unknown flags");
    if (a->max_history < 1 || a->max_history > 4096) return bad("max_history must be 1..4096");
    if (!(a->depth_tol > 0.0f) || !(a->normal_tol > 0.0f)) return bad("depth_tol and normal_tol must be > 0");
    if (a->tiling.num_ranks > 1) return bad("the pass works on a whole frame (tiling.num_ranks > 1)");
    if (a->tiling.local_rows != 0 && a->tiling.local_rows != a->height) return bad("tiling.local_rows is not the frame's height");
    if (!a->color || !a->normal_depth || !a->prim_id) return bad("NULL input plane");
    if (!a->history) return bad("NULL history (the output plane)");
    const bool reset = (a->flags & RT_TEMPORAL_RESET) != 0;
    if (!reset && (!a->prev_history || !a->prev_normal_depth || !a->prev_prim_id))
        return bad("NULL prev_* plane without RT_TEMPORAL_RESET");
    const uint64_t n = (uint64_t)a->width * a->height;
    if (n > 0x7fffffffull) return bad("frame too large");
    if (!reset) {  // (with RT_TEMPORAL_RESET nothing is gathered)
        const void* outs[3] = {a->history, a->motion, a->pos};
        const uint64_t out_bytes[3] = {n * 16u, n * 8u, n * 4u};
        const void* prevs[3] = {a->prev_history, a->prev_normal_depth, a->prev_prim_id};
        const uint64_t prev_bytes[3] = {n * 16u, n * 16u, n * 4u};
        for (int o = 0; o < 3; o++)
            for (int i = 0; i < 3; i++)
                if (overlaps(outs[o], out_bytes[o], prevs[i], prev_bytes[i]))
                    return bad(o == 0 && i == 0 ? "history must not alias prev_history (ping-pong two planes)"
                                                : "an output overlaps a prev_* plane");
    }
    *pixels = n;
    TemporalParams& P = *out;
    P = TemporalParams{};
    P.color = a->color;
    P.normal_depth = a->normal_depth;
    P.prim_id = a->prim_id;
    P.prev_history = reset ? nullptr : a->prev_history;
    P.prev_normal_depth = reset ? nullptr : a->prev_normal_depth;
    P.prev_prim_id = reset ? nullptr : a->prev_prim_id;
    P.history = a->history;
    P.motion = a->motion;
    P.pos = a->pos;
    P.width = a->width;
    P.height = a->height;
    P.flags = a->flags;
    P.max_history = (float)a->max_history;
    P.depth_tol = a->depth_tol;
    P.min_ndot = 1.0f - a->normal_tol;
    P.width_f = (float)a->width;
    P.half_w = (float)a->width / 2.0f;
    P.half_h = (float)a->height / 2.0f;
    P.cur = temporal_camera(a->inputs);
    P.prev = reset ? P.cur : temporal_camera(a->prev_inputs);  // (prev_inputs is not read with RT_TEMPORAL_RESET)
    return RT_OK;
}

int rt_temporal(const rt_temporal_args* a, rt_stream stream) {
    // (every check runs before the first device call)
    TemporalParams P;
    uint64_t n = 0;
    const int rc = temporal_params("rt_temporal", a, &P, &n);
    if (rc || n == 0) return rc;
    return launch_temporal(P, stream);
}

int rt_temporal_dynamic(const rt_temporal_args* a, const float* prim_motion, uint32_t num_prims, rt_stream stream) {
    TemporalParams P;
    uint64_t n = 0;
    const int rc = temporal_params("rt_temporal_dynamic", a, &P, &n);
    if (rc) return rc;
    const auto bad = [](const char* msg) {
        set_error(std::string("rt_temporal_dynamic: ") + msg);
        return (int)RT_ERR_INVALID_ARGUMENT;
    };
    if (!(a->flags & RT_TEMPORAL_RESET)) {  // (with RT_TEMPORAL_RESET the table is never read)
        if (!prim_motion) return bad("NULL prim_motion without RT_TEMPORAL_RESET");
        if ((uintptr_t)prim_motion % 16u) return bad("prim_motion must be 16-byte aligned (float4 entries)");
        const void* outs[3] = {a->history, a->motion, a->pos};
        const uint64_t out_bytes[3] = {n * 16u, n * 8u, n * 4u};
        for (int o = 0; o < 3; o++)
            if (overlaps(outs[o], out_bytes[o], prim_motion, (uint64_t)num_prims * 16u))
                return bad("an output overlaps the prim_motion table");
    }
    if (n == 0) return RT_OK;
    return launch_temporal_dynamic(P, prim_motion, num_prims, stream);
}

int rt_temporal_moments(const rt_temporal_args* a, const float* prim_motion, uint32_t num_prims, const float* prev_moments,
                        float* moments, rt_stream stream) {
    TemporalParams P;
    uint64_t n = 0;
    const int rc = temporal_params("rt_temporal_moments", a, &P, &n);
    if (rc) return rc;
    const auto bad = [](const char* msg) {
        set_error(std::string("rt_temporal_moments: ") + msg);
        return (int)RT_ERR_INVALID_ARGUMENT;
    };
    const bool reset = (a->flags & RT_TEMPORAL_RESET) != 0;
    const bool dynamic = prim_motion != nullptr;  // NULL: rt_temporal's semantics, else rt_temporal_dynamic's
    if (!dynamic && num_prims != 0) return bad("NULL prim_motion with num_prims > 0");
    if (!moments) return bad("NULL moments (the output plane)");
    if (!reset && !prev_moments) return bad("NULL prev_moments without RT_TEMPORAL_RESET");
    const uint64_t table_bytes = (uint64_t)num_prims * 16u;
    const void* outs[3] = {a->history, a->motion, a->pos};
    const uint64_t out_bytes[3] = {n * 16u, n * 8u, n * 4u};
    if (dynamic && !reset) {  // (with RT_TEMPORAL_RESET the table is never read)
        if ((uintptr_t)prim_motion % 16u) return bad("prim_motion must be 16-byte aligned (float4 entries)");
        for (int o = 0; o < 3; o++)
            if (overlaps(outs[o], out_bytes[o], prim_motion, table_bytes)) return bad("an output overlaps the prim_motion table");
    }
    // the moments plane against everything the launch reads or writes
    const void* ins[3] = {a->color, a->normal_depth, a->prim_id};
    const uint64_t in_bytes[3] = {n * 16u, n * 16u, n * 4u};
    for (int i = 0; i < 3; i++)
        if (overlaps(moments, n * 8u, ins[i], in_bytes[i])) return bad("moments overlaps an input plane");
    for (int o = 0; o < 3; o++)
        if (overlaps(moments, n * 8u, outs[o], out_bytes[o])) return bad("moments overlaps another output");
    if (!reset) {
        const void* prevs[4] = {a->prev_history, a->prev_normal_depth, a->prev_prim_id, prev_moments};
        const uint64_t prev_bytes[4] = {n * 16u, n * 16u, n * 4u, n * 8u};
        for (int i = 0; i < 4; i++)
            if (overlaps(moments, n * 8u, prevs[i], prev_bytes[i]))
                return bad(i == 3 ? "moments must not alias prev_moments (ping-pong two planes)" : "moments overlaps a prev_* plane");
        for (int o = 0; o < 3; o++)
            if (overlaps(outs[o], out_bytes[o], prev_moments, n * 8u)) return bad("an output overlaps prev_moments");
        if (dynamic && overlaps(moments, n * 8u, prim_motion, table_bytes)) return bad("moments overlaps the prim_motion table");
    }
    if (n == 0) return RT_OK;
    return launch_temporal_moments(P, dynamic, prim_motion, num_prims, reset ? nullptr : prev_moments, moments, stream);
}

int rt_scene_motion(const rt_hittable_desc* prev, const rt_hittable_desc* cur, uint32_t num_hittables, float* table) {
    if (num_hittables && (!prev || !cur || !table)) {
        set_error("rt_scene_motion: NULL argument with num_hittables > 0");
        return RT_ERR_INVALID_ARGUMENT;
    }
    // (this file is compiled -ffp-contract=off: every operation below is one binary32 rounding)
    for (uint32_t i = 0; i < num_hittables; i++) {
        const rt_hittable_desc& p = prev[i];
        const rt_hittable_desc& c = cur[i];
        float* m = table + (size_t)i * 4;
        m[0] = m[1] = m[2] = m[3] = 0.0f;  // no history
        if (!p.is_active || !c.is_active || p.type != c.type) continue;
        const bool sphere = c.type == RT_SPHERE;
        if (!sphere && c.type != RT_XYRECT && c.type != RT_XZRECT && c.type != RT_YZRECT) continue;
        if (sphere ? !(p.radius > 0.0f && c.radius > 0.0f) : !(p.width == c.width && p.height == c.height)) continue;
        const auto same_bits = [](const float a, const float b) { return std::memcmp(&a, &b, sizeof(float)) == 0; };
        const bool same_size = sphere ? same_bits(p.radius, c.radius)
                                      : same_bits(p.width, c.width) && same_bits(p.height, c.height);
        if (same_size && std::memcmp(p.center, c.center, sizeof(p.center)) == 0) {
            m[3] = 1.0f;  // at rest: exactly (0, 0, 0, 1), which the kernel passes through without arithmetic
            continue;
        }
        const float s = sphere ? p.radius / c.radius : 1.0f;
        for (int k = 0; k < 3; k++) {
            const float scaled = s * c.center[k];
            m[k] = p.center[k] - scaled;
        }
        m[3] = s;
    }
    return RT_OK;
}

int rt_scene_edit(const rt_scene* base, const rt_hittable_desc* hittables, uint32_t num_hittables, rt_scene** out) {
    if (!out) { set_error("rt_scene_edit: out is NULL"); return RT_ERR_INVALID_ARGUMENT; }
    *out = nullptr;
    if (!base || (!hittables && num_hittables)) { set_error("rt_scene_edit: NULL argument"); return RT_ERR_INVALID_ARGUMENT; }
    if (!base->described) {
        set_error("rt_scene_edit: the base scene keeps no description");
        return RT_ERR_UNSUPPORTED;
    }
    if (num_hittables != base->num_hittables) {
        set_error("rt_scene_edit: hittable count " + std::to_string(num_hittables) + " differs from the base scene's " +
                  std::to_string(base->num_hittables) + " (primitive ids would change their meaning)");
        return RT_ERR_INVALID_ARGUMENT;
    }
    return guarded("rt_scene_edit", [&]() -> int {
        rt_scene_desc d;
        d.hittables = hittables;
        d.num_hittables = num_hittables;
        d.materials = base->materials.data();
        d.num_materials = (uint32_t)base->materials.size();
        d.images = base->images.data();
        d.num_images = (uint32_t)base->images.size();
        HostScene h;
        std::string err;
        // the image table must describe the block `base` uploaded: its texel layout, not this thread's current one
        struct Layout {
            const int saved = g_texel_bytes;
            ~Layout() { g_texel_bytes = saved; }
        } layout;
        g_texel_bytes = base->texel_bytes;
        const int rc = build_host_scene(&d, &h, &err, /*with_texels=*/false);
        if (rc) { set_error("rt_scene_edit: " + err); return rc; }
        const int r = create_device_scene(h, out, base->texel_block);
        if (r) return r;
        keep_description(out, d, base->texel_bytes);
        (*out)->texel_block_bytes = base->texel_block_bytes;
        (*out)->dev.device_bytes += base->texel_block_bytes;  // (shared with `base`, counted in both)
        return RT_OK;
    });
}

int rt_scene_destroy(rt_scene* scene) {
    if (!scene) return RT_OK;
    free_device(&scene->dev);
    delete scene;
    return RT_OK;
}

int rt_scene_get_info(const rt_scene* scene, rt_scene_info* info) {
    if (!scene || !info) { set_error("rt_scene_get_info: NULL argument"); return RT_ERR_INVALID_ARGUMENT; }
    info->num_primitives = scene->dev.num_prims;
    info->num_nodes = scene->dev.num_nodes;
    info->num_materials = scene->dev.num_mats;
    info->bvh_depth = scene->dev.depth;
    info->device_bytes = scene->dev.device_bytes;
    return RT_OK;
}

}  // extern "C"
