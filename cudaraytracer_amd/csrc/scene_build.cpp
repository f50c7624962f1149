// scene_build.cpp — host side of the scene boundary: validation, flat-table packing and the BVH build.
//
// Replaces the reference's host-side scene construction: the managed-memory pointer graph of
// CudaLayer::GenerateWorld (CudaLayer.cpp:103-256) and the recursive BVHNode constructor
// (Hittable.cuh:303-385).  The reference splits by hittable type, then in list order (no spatial
// criterion), which costs ~50 box tests per ray on the RTIOW scene.  Here a full-sweep
// SAH build over padded reference boxes produces a BVH with the same closest-hit semantics: the
// primitive tests alone decide the hit, boxes only cull (see rt_internal.h).
#include <algorithm>
#include <limits>
#include <map>
#include <functional>
#include <array>
#include <cmath>
#include <cstring>
#include <numeric>

#include "rt_bounce_entry.h"
#include "rt_internal.h"

// rt_set_bounce_classes' default: 2, the re-paired form (profiles/r14a_ab_bounce_classes.txt); an
// A/B build sets another
#ifndef RT_BOUNCE_CLASSES_DEFAULT
#define RT_BOUNCE_CLASSES_DEFAULT 2
#endif

namespace rt {

thread_local int g_bounce_classes = RT_BOUNCE_CLASSES_DEFAULT;
thread_local uint32_t g_bounce_class_node_limit = 0x7fffu;

namespace {

struct Box {
    float lo[3], hi[3];
    void empty() {
        for (int i = 0; i < 3; i++) { lo[i] = INFINITY; hi[i] = -INFINITY; }
    }
    void grow(const Box& b) {
        for (int i = 0; i < 3; i++) { lo[i] = std::min(lo[i], b.lo[i]); hi[i] = std::max(hi[i], b.hi[i]); }
    }
    float area() const {
        float dx = hi[0] - lo[0], dy = hi[1] - lo[1], dz = hi[2] - lo[2];
        if (!(dx >= 0) || !(dy >= 0) || !(dz >= 0)) return 0.0f;
        return 2.0f * (dx * dy + dy * dz + dz * dx);
    }
};

// Rect plane/extent exactly as XYRect/XZRect/YZRect::Hit compute them (Hittable.cuh:142-147, 198-203,
// 254-259): a0 = c.a - (w / 2) etc.  Evaluated in binary32 so the device sees identical floats.
struct RectGeom { float k, a0, a1, b0, b1; int ia, ib, ik; };
RectGeom rect_geom(const rt_hittable_desc& h) {
    RectGeom g;
    const float* c = h.center;
    volatile float w2 = h.width / 2, h2 = h.height / 2;  // keep binary32 rounding of each step
    if (h.type == RT_XYRECT) {
        g.a0 = c[0] - w2; g.a1 = c[0] + w2; g.b0 = c[1] - h2; g.b1 = c[1] + h2; g.k = c[2];
        g.ia = 0; g.ib = 1; g.ik = 2;
    } else if (h.type == RT_XZRECT) {
        g.a0 = c[0] - w2; g.a1 = c[0] + w2; g.b0 = c[2] - h2; g.b1 = c[2] + h2; g.k = c[1];
        g.ia = 0; g.ib = 2; g.ik = 1;
    } else {  // YZ: y from height, z from width
        g.a0 = c[1] - h2; g.a1 = c[1] + h2; g.b0 = c[2] - w2; g.b1 = c[2] + w2; g.k = c[0];
        g.ia = 1; g.ib = 2; g.ik = 0;
    }
    return g;
}

// Reference primitive box (Hittable.cuh:112-116, 171-181, 227-237, 283-293), grown outward.
Box prim_box(const rt_hittable_desc& h) {
    Box b;
    if (h.type == RT_SPHERE) {
        for (int i = 0; i < 3; i++) { b.lo[i] = h.center[i] - h.radius; b.hi[i] = h.center[i] + h.radius; }
    } else {
        RectGeom g = rect_geom(h);
        b.lo[g.ia] = g.a0; b.hi[g.ia] = g.a1;
        b.lo[g.ib] = g.b0; b.hi[g.ib] = g.b1;
        b.lo[g.ik] = g.k - 0.0001f; b.hi[g.ik] = g.k + 0.0001f;
    }
    for (int i = 0; i < 3; i++) {
        float m = std::max(std::fabs(b.lo[i]), std::fabs(b.hi[i]));
        float pad = 1e-5f * m + 1e-6f;
        b.lo[i] -= pad;
        b.hi[i] += pad;
    }
    return b;
}

// v with the low byte of its binary32 representation replaced by `payload`, moved outward: the result is <= v
// (up = false) or >= v (up = true).  Works on the magnitude, whose bit pattern orders like the value; a zero
// or tiny magnitude crosses to the other sign's side (a denormal of the right sign).
float with_low_byte(float v, uint32_t payload, bool up) {
    uint32_t b;
    std::memcpy(&b, &v, 4);
    const uint32_t sign = b & 0x80000000u, mag = b & 0x7fffffffu;
    const bool grow = (sign == 0) == up;  // the magnitude must not shrink (else: must not grow)
    uint32_t out;
    // (a plane at the float range's end keeps its magnitude just under FLT_MAX: no finite ray reaches past it)
    if (grow) {
        out = sign | (((mag >> 8) + 1u) << 8) | payload;  // > mag
    } else if ((mag >> 8) > 0u) {
        out = sign | (((mag >> 8) - 1u) << 8) | payload;  // < mag
    } else {
        out = (sign ^ 0x80000000u) | 0x100u | payload;  // |v| < 256 ulps of 2^-149: a denormal past zero
    }
    if ((out & 0x7fffffffu) >= 0x7f7fff00u) out = (out & 0x80000000u) | 0x7f7fff00u | payload;  // stay finite
    float r;
    std::memcpy(&r, &out, 4);
    return r;
}

struct BuildPrim {
    Box box;
    float centroid[3];
    int src;  // index into desc.hittables
};

struct Builder {
    int leaf_max = kLeafMax;
    float traversal = 1.6f;  // SAH: node visit cost / primitive test cost
    std::vector<BuildPrim> prims;
    std::vector<int> order;  // final primitive order
    struct Node {
        Box box[2];
        int child[2];
    };
    std::vector<Node> nodes;
    uint32_t max_depth = 0;
    // > 0: every leaf at a depth <= depth_limit (root = 1).  Each split then keeps both sides within what a
    // subtree of the remaining depth can hold (leaf_max << levels left), choosing the best SAH split among those.
    uint32_t depth_limit = 0;

    Box range_box(int b, int e) const {
        Box r;
        r.empty();
        for (int i = b; i < e; i++) r.grow(prims[order[i]].box);
        return r;
    }

    // leaf reference: ~(first << 2 | (count - 1)), count in 1..4 (rt_internal.h)
    int make_leaf(int b, int e) const { return ~((b << 2) | (e - b - 1)); }

    // Returns the child reference for [b, e).
    int build(int b, int e, uint32_t depth) {
        int n = e - b;
        if (depth > max_depth) max_depth = depth;
        const bool must_split = depth == 1;  // the root is always an internal node (see build_root)
        if (n <= 1 && !must_split) return make_leaf(b, e);
        int lo_split = 1, hi_split = n - 1;  // allowed left-side sizes
        if (depth_limit) {
            if (depth >= depth_limit) return make_leaf(b, e);  // n <= leaf_max here by the capacities above
            const int64_t cap = (int64_t)leaf_max << (depth_limit - depth - 1);
            lo_split = (int)std::max<int64_t>(1, n - cap);
            hi_split = (int)std::min<int64_t>(n - 1, cap);
        }
        // Full-sweep SAH over the three centroid axes.
        float best_cost = INFINITY;
        int best_axis = -1, best_split = -1;
        std::vector<int> tmp(order.begin() + b, order.begin() + e);
        std::vector<float> right_area(n);
        for (int axis = 0; axis < 3; axis++) {
            std::stable_sort(tmp.begin(), tmp.end(), [&](int x, int y) {
                return prims[x].centroid[axis] < prims[y].centroid[axis];
            });
            Box acc;
            acc.empty();
            for (int i = n - 1; i > 0; i--) {
                acc.grow(prims[tmp[i]].box);
                right_area[i] = acc.area();
            }
            acc.empty();
            for (int i = 1; i < n; i++) {
                acc.grow(prims[tmp[i - 1]].box);
                if (i < lo_split || i > hi_split) continue;
                float cost = acc.area() * (float)i + right_area[i] * (float)(n - i);
                if (cost < best_cost) { best_cost = cost; best_axis = axis; best_split = i; }
            }
        }
        Box all = range_box(b, e);
        float leaf_cost = all.area() * (float)n;
        if (!must_split && n <= leaf_max && best_cost + traversal * all.area() >= leaf_cost) return make_leaf(b, e);
        if (best_axis < 0) {  // every candidate cost overflowed (boxes at the end of the float range): object median
            best_axis = 0;
            best_split = std::min(std::max(n / 2, lo_split), hi_split);
        }
        std::stable_sort(order.begin() + b, order.begin() + e, [&](int x, int y) {
            return prims[x].centroid[best_axis] < prims[y].centroid[best_axis];
        });
        int mid = b + best_split;
        int id = (int)nodes.size();
        nodes.push_back(Node());
        int l = build(b, mid, depth + 1);
        int r = build(mid, e, depth + 1);
        nodes[id].child[0] = l;
        nodes[id].child[1] = r;
        nodes[id].box[0] = range_box(b, mid);
        nodes[id].box[1] = range_box(mid, e);
        return id;
    }

    void build_root() {
        nodes.clear();
        max_depth = 0;
        int n = (int)prims.size();
        order.resize(n);
        std::iota(order.begin(), order.end(), 0);
        if (n == 0) return;
        if (n == 1) {
            // Root with both children referencing the single leaf (a second test of the same primitive
            // cannot change the closest hit: Sphere::Hit is strict in t_max, rects re-accept the same t).
            nodes.push_back(Node());
            nodes[0].child[0] = nodes[0].child[1] = make_leaf(0, 1);
            nodes[0].box[0] = nodes[0].box[1] = prims[0].box;
            max_depth = 2;
            return;
        }
        max_depth = 1;
        int r = build(0, n, 1);
        (void)r;  // n >= 2 always yields an internal root at index 0
    }
};

// The 32-B primitive record (rt_internal.h).
void pack_prim(const rt_hittable_desc& h, float* o) {
    uint32_t tag = (uint32_t)h.type | ((uint32_t)h.material << 4);
    if (h.type == RT_SPHERE) {
        o[0] = h.center[0]; o[1] = h.center[1]; o[2] = h.center[2]; o[3] = h.radius;
        // o[5]: RN(1/radius) for the kernel's fast normal division (render.hip divs_rn), 0 = IEEE division
        const float ar = std::fabs(h.radius);
        o[4] = h.radius * h.radius; o[5] = (ar >= 0x1p-40f && ar <= 0x1p40f) ? 1.0f / h.radius : 0.0f; o[6] = 0.0f;
    } else {
        RectGeom g = rect_geom(h);
        o[0] = g.k; o[1] = g.a0; o[2] = g.a1; o[3] = g.b0;
        o[4] = g.b1; o[5] = 0.0f; o[6] = 0.0f;
    }
    o[7] = bits_to_float(tag);
}

// The 64-B node record (rt_internal.h).
void pack_node16(const Builder::Node& n, float* o) {
    o[0] = n.box[0].lo[0]; o[1] = n.box[0].hi[0]; o[2] = n.box[0].lo[1]; o[3] = n.box[0].hi[1];
    o[4] = n.box[1].lo[0]; o[5] = n.box[1].hi[0]; o[6] = n.box[1].lo[1]; o[7] = n.box[1].hi[1];
    o[8] = n.box[0].lo[2]; o[9] = n.box[0].hi[2]; o[10] = n.box[1].lo[2]; o[11] = n.box[1].hi[2];
    o[12] = bits_to_float((uint32_t)n.child[0]);
    o[13] = bits_to_float((uint32_t)n.child[1]);
    o[14] = 0.0f;
    o[15] = 0.0f;
}

// The 48-B node record: the three box float4 of the 64-B one.  The child references also ride in the low bytes of the
// planes (lo_x, hi_x of each child: bits 0-15; wide: lo_y, hi_y: bits 16-31), so a lane's three 16-B box loads carry
// them and the vector path needs no fourth load (render.hip).  Each carrier plane moves outward by < 512 ulps (lo
// down, hi up): the box only grows, and the culling stays conservative.
void pack_node48(const Builder::Node& n, const bool wide, float* o48) {
    float o[16];
    pack_node16(n, o);
    for (int k = 0; k < 12; k++) o48[k] = o[k];
    for (int c = 0; c < 2; c++) {
        const uint32_t r = (uint32_t)n.child[c];
        float* q = o48 + 4 * c;  // lo_x, hi_x, lo_y, hi_y of child c
        q[0] = with_low_byte(q[0], r & 0xffu, false);
        q[1] = with_low_byte(q[1], (r >> 8) & 0xffu, true);
        if (wide) {
            q[2] = with_low_byte(q[2], (r >> 16) & 0xffu, false);
            q[3] = with_low_byte(q[3], r >> 24, true);
        }
    }
}

// Bounce entries (rt_bounce_entry.h): the chain nodes behind the real ones in nodes48 / refs, one record per leaf and
// the origin grid.  16-bit-reference scenes whose real + chain nodes stay below 0x7fff; else no table.
void build_bounce_entries(const Builder& B, HostScene* out) {
    const uint32_t N = out->num_nodes;
    if (out->wide_refs || N == 0) return;
    struct Step { int node, side; };
    struct Leaf { int ref; std::vector<Step> path; Box box; };
    std::vector<Leaf> leaves;
    std::vector<uint32_t> height(N, 0u);  // internal nodes on the longest way down from a node, itself counted
    {
        std::vector<Step> path;
        std::function<uint32_t(int)> walk = [&](const int n) -> uint32_t {
            uint32_t h = 0;
            for (int side = 0; side < 2; side++) {
                path.push_back(Step{n, side});
                const int c = B.nodes[n].child[side];
                if (c < 0) leaves.push_back(Leaf{c, path, B.nodes[n].box[side]});
                else h = std::max(h, walk(c));
                path.pop_back();
            }
            return height[n] = h + 1u;
        };
        walk(0);
    }
    const auto ref_height = [&](const int r) { return r < 0 ? 0u : height[r]; };
    // chain node (A_2k, side of its on-path child): children S_2k (off A_2k) and S_2k-1 (off A_2k-1)
    std::vector<Builder::Node> chain;
    std::vector<int> chain_of((size_t)N * 2, -1);
    std::vector<std::array<uint32_t, kTileEntryMax>> records;
    for (const Leaf& L : leaves) {
        const size_t a = L.path.size();
        std::vector<int> refs;  // behind the own leaf, from the deepest up
        const auto sibling = [&](const size_t i) { return B.nodes[L.path[i].node].child[1 - L.path[i].side]; };  // S_(i+1)
        if (a & 1u) refs.push_back(sibling(a - 1));
        for (size_t k = a / 2; k >= 1; k--) {
            const Step& lo = L.path[2 * k - 1];  // A_2k
            const Step& up = L.path[2 * k - 2];  // A_2k-1
            int& id = chain_of[(size_t)lo.node * 2 + (size_t)lo.side];
            if (id < 0) {
                id = (int)(N + chain.size());
                Builder::Node c;
                c.child[0] = B.nodes[lo.node].child[1 - lo.side];
                c.box[0] = B.nodes[lo.node].box[1 - lo.side];
                c.child[1] = B.nodes[up.node].child[1 - up.side];
                c.box[1] = B.nodes[up.node].box[1 - up.side];
                chain.push_back(c);
            }
            refs.push_back(id);
        }
        std::array<uint32_t, kTileEntryMax> e;
        e.fill(kTileEntryNone);
        // The kernel's stack holds out->depth entries above its pads.  Reference j (0 = first) is visited with
        // m - 1 - j entries below it; a visit with h entries below writes entry h, and a subtree of `height` internal
        // levels under it reaches entry h + height - 1 (a chain node's near child is visited one entry higher).
        const size_t m = refs.size();
        bool fits = m <= kBounceChainMax && m >= 1 && m - 1 <= out->depth;
        for (size_t j = 0; j < m && fits; j++) {
            const uint32_t h = (uint32_t)(m - 1 - j);
            uint32_t top = 0;  // the highest entry written, + 1
            if (refs[j] >= (int)N) {
                const Builder::Node& c = chain[(size_t)refs[j] - N];
                top = h + 1u + std::max(ref_height(c.child[0]), ref_height(c.child[1]));
            } else if (refs[j] >= 0) {
                top = h + height[refs[j]];
            }
            fits = top <= out->depth;
        }
        if (fits) {
            e[0] = (uint32_t)L.ref & 0xffffu;
            for (size_t j = 0; j < m; j++) e[1 + j] = (uint32_t)refs[j] & 0xffffu;
        } else {
            e[0] = kTileEntryRoot;
        }
        records.push_back(e);
    }
    if (N + chain.size() >= 0x7fffu || records.size() > 0xffffu) return;

    // The origin grid over the non-spanning primitives' boxes
    Box scene;
    scene.empty();
    for (const BuildPrim& p : B.prims) scene.grow(p.box);
    const auto spanning = [&](const BuildPrim& p) {
        int wide_axes = 0;
        for (int i = 0; i < 3; i++)
            if (p.box.hi[i] - p.box.lo[i] > 0.5f * (scene.hi[i] - scene.lo[i])) wide_axes++;
        return wide_axes >= 2;
    };
    Box g;
    g.empty();
    std::vector<char> candidate(leaves.size(), 0);  // the leaf holds a non-spanning primitive
    bool any = false;
    for (size_t l = 0; l < leaves.size(); l++) {
        const uint32_t r = ~(uint32_t)leaves[l].ref, first = r >> 2, count = (r & 3u) + 1u;
        for (uint32_t i = first; i < first + count; i++) {
            const BuildPrim& p = B.prims[B.order[i]];
            if (spanning(p)) continue;
            g.grow(p.box);
            candidate[l] = 1;
            any = true;
        }
    }
    if (!any) {  // every primitive spans: the grid covers the scene, every leaf is a candidate
        g = scene;
        std::fill(candidate.begin(), candidate.end(), 1);
    }
    float ext[3];
    double volume = 1.0;
    int flat_axes = 0;
    for (int i = 0; i < 3; i++) {
        ext[i] = g.hi[i] - g.lo[i];
        if (!(ext[i] > 0.0f) || !std::isfinite(ext[i])) { ext[i] = 0.0f; flat_axes++; }
        else volume *= (double)ext[i];
    }
    if (!std::isfinite(g.lo[0]) || !std::isfinite(g.lo[1]) || !std::isfinite(g.lo[2]) || !std::isfinite(volume)) return;
    const double target = (double)std::min<size_t>(kBounceGridMaxCells, std::max<size_t>(1, 4 * leaves.size()));
    double edge = flat_axes == 3 ? 1.0 : std::pow(volume / target, 1.0 / (double)(3 - flat_axes));
    uint32_t dim[3];
    for (;;) {
        uint64_t cells = 1;
        for (int i = 0; i < 3; i++) {
            const double d = ext[i] > 0.0f && edge > 0.0 ? std::ceil((double)ext[i] / edge) : 1.0;
            dim[i] = (uint32_t)std::min(std::max(d, 1.0), 256.0);
            cells *= dim[i];
        }
        if (cells <= kBounceGridMaxCells) break;
        edge *= 1.1;
    }
    for (int i = 0; i < 3; i++) {
        out->grid_dim[i] = dim[i];
        out->grid_origin[i] = g.lo[i];
        out->grid_inv[i] = ext[i] > 0.0f ? (float)dim[i] / ext[i] : 0.0f;
        if (!std::isfinite(out->grid_inv[i])) out->grid_inv[i] = 0.0f;
        out->grid_off[i] = -(g.lo[i] * out->grid_inv[i]);
    }
    out->bounce_grid.resize((size_t)dim[0] * dim[1] * dim[2]);
    for (uint32_t z = 0; z < dim[2]; z++)
        for (uint32_t y = 0; y < dim[1]; y++)
            for (uint32_t x = 0; x < dim[0]; x++) {
                const uint32_t cell[3] = {x, y, z};
                float c[3];
                for (int i = 0; i < 3; i++)
                    c[i] = out->grid_inv[i] > 0.0f ? g.lo[i] + ((float)cell[i] + 0.5f) / out->grid_inv[i] : g.lo[i];
                size_t best = 0;
                float best_area = INFINITY, best_dist = INFINITY;
                for (size_t l = 0; l < leaves.size(); l++) {
                    if (!candidate[l]) continue;
                    const Box& b = leaves[l].box;
                    float d2 = 0.0f;
                    for (int i = 0; i < 3; i++) {
                        const float d = std::max(std::max(b.lo[i] - c[i], c[i] - b.hi[i]), 0.0f);
                        d2 += d * d;
                    }
                    const float area = b.area();
                    // a containing box beats any other; among those the smallest, else the nearest
                    if (d2 < best_dist || (d2 == best_dist && area < best_area)) {
                        best = l;
                        best_dist = d2;
                        best_area = area;
                    }
                }
                out->bounce_grid[((size_t)z * dim[1] + y) * dim[0] + x] = (uint16_t)best;
            }

    // Direction classes (rt_bounce_entry.h): per record and class the siblings a ray of the class can reach from the
    // record's region; form 2 appends its pairs to `chain`, behind the num_chain nodes of the full records
    const size_t num_chain = chain.size();
    bool flat_axis = false;
    for (int i = 0; i < 3; i++) flat_axis = flat_axis || !(out->grid_inv[i] > 0.0f);
    if (g_bounce_classes != 0 && !flat_axis) {
        const size_t R = records.size();
        std::vector<double>& reg = out->class_regions;
        reg.resize(R * 6);
        for (size_t r = 0; r < R; r++)
            for (int i = 0; i < 3; i++) { reg[6 * r + i] = INFINITY; reg[6 * r + 3 + i] = -INFINITY; }
        for (uint32_t z = 0; z < dim[2]; z++)
            for (uint32_t y = 0; y < dim[1]; y++)
                for (uint32_t x = 0; x < dim[0]; x++) {
                    const uint32_t cell[3] = {x, y, z};
                    double* q = reg.data() + 6 * (size_t)out->bounce_grid[((size_t)z * dim[1] + y) * dim[0] + x];
                    for (int i = 0; i < 3; i++) {
                        // the origins whose exact o * inv + off lies in [cell, cell + 1); a border cell one cell further
                        const double inv = (double)out->grid_inv[i], off = (double)out->grid_off[i];
                        const double lo = ((cell[i] == 0 ? -1.0 : (double)cell[i]) - off) / inv;
                        const double hi = ((cell[i] + 1u == dim[i] ? (double)dim[i] + 1.0 : (double)cell[i] + 1.0) - off) / inv;
                        q[i] = std::min(q[i], lo);
                        q[3 + i] = std::max(q[3 + i], hi);
                    }
                }
        // whether a subtree holds a spanning primitive (every primitive counts as one where all of them span)
        std::vector<signed char> span_node(N, -1);
        std::function<bool(int)> spans = [&](const int ref) -> bool {
            if (ref < 0) {
                if (!any) return true;
                const uint32_t r = ~(uint32_t)ref, first = r >> 2, count = (r & 3u) + 1u;
                for (uint32_t i = first; i < first + count; i++)
                    if (spanning(B.prims[B.order[i]])) return true;
                return false;
            }
            if (span_node[ref] < 0) {
                const bool a = spans(B.nodes[ref].child[0]), b = spans(B.nodes[ref].child[1]);
                span_node[ref] = a || b;
            }
            return span_node[ref] != 0;
        };
        const auto reachable = [](const double* Rg, const Box& S, const uint32_t cls) -> bool {
            const uint32_t k = cls >> 3;
            double D = 0.0, A = 0.0;
            for (int j = 0; j < 3; j++) {
                const double slo = (double)S.lo[j], shi = (double)S.hi[j], rlo = Rg[j], rhi = Rg[3 + j];
                D += (rhi > shi ? rhi : shi) - (rlo < slo ? rlo : slo);
                double a = rlo < 0.0 ? -rlo : rlo;
                const double b = rhi < 0.0 ? -rhi : rhi, c = slo < 0.0 ? -slo : slo, d = shi < 0.0 ? -shi : shi;
                a = a > b ? a : b;
                a = a > c ? a : c;
                A += a > d ? a : d;
            }
            const double m = 0x1p-8 * D + 0x1p-18 * A;
            if (!(m - m == 0.0)) return true;  // (a box that is not finite stays)
            const bool neg_k = (cls >> k & 1u) != 0;
            const double s = neg_k ? Rg[3 + k] - (double)S.lo[k] : (double)S.hi[k] - Rg[k];
            if (s < -m) return false;
            for (uint32_t j = 0; j < 3; j++) {
                if (j == k) continue;
                const bool neg = (cls >> j & 1u) != 0;
                const double lo = neg ? Rg[j] - s - m : Rg[j], hi = neg ? Rg[3 + j] : Rg[3 + j] + s + m;
                if ((double)S.hi[j] < lo - m || (double)S.lo[j] > hi + m) return false;
            }
            return true;
        };
        std::vector<uint32_t>& cr = out->class_records;
        for (uint32_t form = (uint32_t)g_bounce_classes;; form = 1) {
            chain.resize(num_chain);
            cr.assign(R * kBounceClasses * 4, 0u);
            std::map<std::pair<int, int>, int> pair_id;
            for (size_t i = 0; i < num_chain; i++) pair_id[{chain[i].child[0], chain[i].child[1]}] = (int)(N + i);
            for (size_t l = 0; l < R; l++) {
                const Leaf& L = leaves[l];
                const size_t a = L.path.size();
                const double* Rg = reg.data() + 6 * l;
                const bool whole = records[l][0] == kTileEntryRoot || !(Rg[0] <= Rg[3]);
                const auto sib_ref = [&](const size_t i) { return B.nodes[L.path[i].node].child[1 - L.path[i].side]; };
                const auto sib_box = [&](const size_t i) -> const Box& { return B.nodes[L.path[i].node].box[1 - L.path[i].side]; };
                for (uint32_t cls = 0; cls < kBounceClasses; cls++) {
                    std::array<uint32_t, kTileEntryMax> e = records[l];
                    if (!whole && cls != kBounceClassFull) {
                        std::vector<char> reach(a);
                        for (size_t i = 0; i < a; i++) reach[i] = spans(sib_ref(i)) || reachable(Rg, sib_box(i), cls);
                        std::vector<int> refs;  // behind the own leaf, from the deepest up
                        if (form == 1) {
                            if ((a & 1u) && reach[a - 1]) refs.push_back(sib_ref(a - 1));
                            for (size_t k = a / 2; k >= 1; k--)
                                if (reach[2 * k - 1] || reach[2 * k - 2])
                                    refs.push_back(chain_of[(size_t)L.path[2 * k - 1].node * 2 + (size_t)L.path[2 * k - 1].side]);
                        } else {
                            std::vector<size_t> kept;  // from the root
                            for (size_t i = 0; i < a; i++)
                                if (reach[i]) kept.push_back(i);
                            if (kept.size() & 1u) refs.push_back(sib_ref(kept.back()));
                            for (size_t k = kept.size() / 2; k >= 1; k--) {
                                const size_t lo = kept[2 * k - 1], up = kept[2 * k - 2];  // the deeper one is child 0
                                int& id = pair_id[{sib_ref(lo), sib_ref(up)}];
                                if (id == 0) {  // (no chain node has index 0: N >= 1)
                                    id = (int)(N + chain.size());
                                    Builder::Node c;
                                    c.child[0] = sib_ref(lo);
                                    c.box[0] = sib_box(lo);
                                    c.child[1] = sib_ref(up);
                                    c.box[1] = sib_box(up);
                                    chain.push_back(c);
                                }
                                refs.push_back(id);
                            }
                        }
                        // the stack simulation of the full records
                        const size_t m = refs.size();
                        bool fits = m <= kBounceChainMax && (m == 0 || m - 1 <= out->depth);
                        for (size_t j = 0; j < m && fits; j++) {
                            const uint32_t h = (uint32_t)(m - 1 - j);
                            uint32_t top = 0;
                            if (refs[j] >= (int)N) {
                                const Builder::Node& c = chain[(size_t)refs[j] - N];
                                top = h + 1u + std::max(ref_height(c.child[0]), ref_height(c.child[1]));
                            } else if (refs[j] >= 0) {
                                top = h + height[refs[j]];
                            }
                            fits = top <= out->depth;
                        }
                        if (fits) {
                            e.fill(kTileEntryNone);
                            e[0] = (uint32_t)L.ref & 0xffffu;
                            for (size_t j = 0; j < m; j++) e[1 + j] = (uint32_t)refs[j] & 0xffffu;
                        }
                    }
                    uint32_t* w = cr.data() + (l * kBounceClasses + cls) * 4;
                    for (int i = 0; i < 4; i++) w[i] = e[2 * i] | (e[2 * i + 1] << 16);
                }
            }
            if (form == 2 && N + chain.size() >= g_bounce_class_node_limit) continue;  // fall back to form 1
            out->bounce_classes = form;
            break;
        }
        out->num_class_nodes = (uint32_t)(chain.size() - num_chain);
    }

    out->num_chain_nodes = (uint32_t)num_chain;
    out->chain_nodes.resize(num_chain * 16);
    out->nodes48.resize((size_t)(N + chain.size()) * 12);
    out->refs.resize((size_t)N + chain.size());
    for (size_t i = 0; i < chain.size(); i++) {
        if (i < num_chain) pack_node16(chain[i], out->chain_nodes.data() + i * 16);
        pack_node48(chain[i], false, out->nodes48.data() + (N + i) * 12);
        out->refs[N + i] = ((uint32_t)chain[i].child[0] & 0xffffu) | ((uint32_t)chain[i].child[1] << 16);
    }
    out->leaf_records.resize(records.size() * 4);
    for (size_t i = 0; i < records.size(); i++)
        for (int w = 0; w < 4; w++) out->leaf_records[4 * i + w] = records[i][2 * w] | (records[i][2 * w + 1] << 16);
}

// The reference BVH over objs[b, e) exactly as the BVHNode constructor builds it (Hittable.cuh:303-385): the range is
// sorted by type; a span of 1 or 2 becomes a node with primitive children (a span-1 node holds its object twice), a
// larger span splits at the end of the first type group (or in the middle) into two node children.  Node boxes are
// the reference's: primitive boxes (Hittable.cuh:112-116, 171-181, 227-237, 283-293, not padded further) merged by
// SurroundingBox (AABB.cuh:53-62).  Children: >= 0 node index, < 0 ~(desc index).  Returns the node index.
struct RefNode {
    float lo[3], hi[3];
    int child[2];
    uint32_t depth;
};
void ref_prim_box(const rt_hittable_desc& h, float lo[3], float hi[3]) {
    if (h.type == RT_SPHERE) {
        for (int i = 0; i < 3; i++) {
            volatile float c = h.center[i], r = h.radius;
            lo[i] = c - r;
            hi[i] = c + r;
        }
        return;
    }
    RectGeom g = rect_geom(h);
    lo[g.ia] = g.a0; hi[g.ia] = g.a1;
    lo[g.ib] = g.b0; hi[g.ib] = g.b1;
    volatile float k = g.k;
    lo[g.ik] = k - 0.0001f;
    hi[g.ik] = k + 0.0001f;
}

// The flat kernels' exactness check (render.hip flat_trace) per flat record: (lo.xyz, kl), (hi.xyz, kh) — the record's
// own reference box, except that a rectangle's plane axis holds 1e30 in lo/hi (its faces are checked through the
// slab distances instead, kl / kh = k -/+ 0.0001f as AABB::Hit has them) and a sphere's kl / kh are NaN (no plane).
void pack_flat_box(const rt_hittable_desc& h, float* o) {
    float lo[3], hi[3];
    ref_prim_box(h, lo, hi);
    float kl = std::numeric_limits<float>::quiet_NaN(), kh = kl;
    if (h.type != RT_SPHERE) {
        const RectGeom g = rect_geom(h);
        kl = lo[g.ik];
        kh = hi[g.ik];
        lo[g.ik] = hi[g.ik] = 1e30f;
    }
    o[0] = lo[0]; o[1] = lo[1]; o[2] = lo[2]; o[3] = kl;
    o[4] = hi[0]; o[5] = hi[1]; o[6] = hi[2]; o[7] = kh;
}
// The BVH kernels' exactness check (render.hip bvh_clear) per BVH-order primitive: (lo.xyz, 0), (hi.xyz, 0) — its own
// reference box as the reference's BoundingBox computes it (the innermost box on its path through the reference tree)
void pack_ref_box(const rt_hittable_desc& h, float* o) {
    float lo[3], hi[3];
    ref_prim_box(h, lo, hi);
    o[0] = lo[0]; o[1] = lo[1]; o[2] = lo[2]; o[3] = 0.0f;
    o[4] = hi[0]; o[5] = hi[1]; o[6] = hi[2]; o[7] = 0.0f;
}
int build_reference_tree(const rt_hittable_desc* h, std::vector<int>& objs, int b, int e, uint32_t depth,
                         std::vector<RefNode>* nodes) {
    const int id = (int)nodes->size();
    nodes->push_back(RefNode());
    // (a range already in type order — every range below the root, whose sort left it so — is its own stable sort:
    // skipped, so a scene of n primitives builds in O(n log n))
    const auto by_type = [&](int x, int y) { return h[x].type < h[y].type; };
    if (!std::is_sorted(objs.begin() + b, objs.begin() + e, by_type))
        std::stable_sort(objs.begin() + b, objs.begin() + e, by_type);
    const int span = e - b;
    int c0, c1;
    if (span <= 2) {
        c0 = ~objs[b];
        c1 = ~objs[span == 1 ? b : b + 1];
    } else {
        int mid = b;
        while (mid < e && h[objs[mid]].type == h[objs[b]].type) mid++;
        if (mid == b || mid == e) mid = b + span / 2;
        c0 = build_reference_tree(h, objs, b, mid, depth + 1, nodes);
        c1 = build_reference_tree(h, objs, mid, e, depth + 1, nodes);
    }
    float lo[2][3], hi[2][3];
    const int ch[2] = {c0, c1};
    for (int k = 0; k < 2; k++) {
        if (ch[k] >= 0) {
            for (int i = 0; i < 3; i++) { lo[k][i] = (*nodes)[ch[k]].lo[i]; hi[k][i] = (*nodes)[ch[k]].hi[i]; }
        } else {
            ref_prim_box(h[~ch[k]], lo[k], hi[k]);
        }
    }
    RefNode& n = (*nodes)[id];
    for (int i = 0; i < 3; i++) {
        n.lo[i] = std::fmin(lo[0][i], lo[1][i]);
        n.hi[i] = std::fmax(hi[0][i], hi[1][i]);
    }
    n.child[0] = c0;
    n.child[1] = c1;
    n.depth = depth;
    return id;
}

// BVHNode::Hit (Hittable.cuh:387-439) pops the right child before the left one: the order in which it tests the
// primitives, box culling aside (culling skips primitives, never reorders them).
void reference_test_order(const std::vector<RefNode>& nodes, int n, std::vector<int>* out) {
    const RefNode& r = nodes[n];
    if (r.child[0] < 0) {
        out->push_back(~r.child[0]);
        if (r.child[1] != r.child[0]) out->push_back(~r.child[1]);
        return;
    }
    reference_test_order(nodes, r.child[1], out);
    reference_test_order(nodes, r.child[0], out);
}

int check_texture(const rt_texture_desc& t, uint32_t num_images, std::string* err) {
    if (t.type < RT_CONSTANT || t.type > RT_IMAGE) {
        *err = "texture type " + std::to_string(t.type) + " is not CONSTANT/CHECKER/IMAGE";
        return RT_ERR_INVALID_SCENE;
    }
    if (t.type == RT_IMAGE && (t.image < -1 || t.image >= (int32_t)num_images)) {
        *err = "image texture index " + std::to_string(t.image) + " out of range";
        return RT_ERR_INVALID_SCENE;
    }
    return RT_OK;
}

}  // namespace

thread_local int g_leaf_max = kLeafMax;
thread_local int g_sah_traversal_x10 = 16;  // 1.6: C3 −4.4 %, C2 −0.4 % against 1.2 (profiles/r02e_ab_sah.txt)
thread_local int g_texel_bytes = 3;

int pack_materials(const rt_material_desc* mats, uint32_t n, uint32_t num_images, std::vector<float>* out,
                   std::string* err) {
    out->assign((size_t)n * 12, 0.0f);
    for (uint32_t i = 0; i < n; i++) {
        const rt_material_desc& m = mats[i];
        if (m.type < RT_LAMBERTIAN || m.type > RT_DIFFUSELIGHT) {
            *err = "material " + std::to_string(i) + ": type " + std::to_string(m.type) + " invalid";
            return RT_ERR_INVALID_SCENE;
        }
        if (m.type != RT_DIELECTRIC) {
            int rc = check_texture(m.albedo, num_images, err);
            if (rc) { *err = "material " + std::to_string(i) + ": " + *err; return rc; }
        }
        float* o = out->data() + (size_t)i * 12;
        uint32_t tex_type = m.type == RT_DIELECTRIC ? 0u : (uint32_t)m.albedo.type;
        o[0] = bits_to_float((uint32_t)m.type | (tex_type << 4));
        o[1] = m.type == RT_METAL ? m.fuzz : (m.type == RT_DIELECTRIC ? m.ir : 0.0f);
        o[2] = (float)m.light_intensity;  // `light_intensity * value`: int → float (Material.cuh:168)
        int32_t img = m.albedo.type == RT_IMAGE ? m.albedo.image : -1;
        o[3] = bits_to_float((uint32_t)img);
        for (int c = 0; c < 3; c++) {
            o[4 + c] = m.albedo.color[c];
            o[8 + c] = m.albedo.color2[c];
        }
        if (m.type == RT_DIELECTRIC) {
            // ir-only terms of Dielectric::Scatter, with the kernel's binary32 operations (this file is
            // compiled -ffp-contract=off): 1.0f / ir (Material.cuh:124) and Reflectance's r0² (:142-143)
            volatile float ir = m.ir;
            volatile float inv = 1.0f / ir;
            volatile float r0 = (1.0f - ir) / (1.0f + ir);
            volatile float r0sq = r0 * r0;
            o[4] = inv;
            o[5] = r0sq;
            o[6] = 0.0f;
        }
    }
    return RT_OK;
}

void build_light_table(HostScene* h) {
    h->lights.clear();
    h->light_table.clear();
    const size_t nr = h->rects.size() / 8;
    if (nr == 0) return;
    h->light_table.assign(nr * 8 + std::max(h->num_prims, 1u), 0u);
    uint32_t* const flag = h->light_table.data() + nr * 8;
    for (size_t r = 0; r < nr; r++) {
        const uint32_t* e = h->rects.data() + r * 8;
        const float width = bits_to_float(e[3]), height = bits_to_float(e[4]);
        const float* m0 = h->mats.data() + (size_t)e[6] * 12;
        uint32_t mword;
        std::memcpy(&mword, m0, 4);
        if (!(width > 0.0f) || !(height > 0.0f) || (mword & 15u) != (uint32_t)RT_DIFFUSELIGHT || !(m0[2] > 0.0f)) continue;
        uint32_t* o = h->light_table.data() + h->lights.size() * 8;
        for (int k = 0; k < 6; k++) o[k] = e[k];
        flag[e[5]] = 1u;
        h->lights.push_back(e[7]);
    }
}

int build_host_scene(const rt_scene_desc* desc, HostScene* out, std::string* err, bool with_texels) {
    if (!desc) { *err = "scene description is NULL"; return RT_ERR_INVALID_ARGUMENT; }
    if ((desc->num_hittables && !desc->hittables) || (desc->num_materials && !desc->materials) ||
        (desc->num_images && !desc->images)) {
        *err = "scene description has a NULL array with a non-zero count";
        return RT_ERR_INVALID_ARGUMENT;
    }
    *out = HostScene();
    int rc = pack_materials(desc->materials, desc->num_materials, desc->num_images, &out->mats, err);
    if (rc) return rc;
    out->num_mats = desc->num_materials;
    for (uint32_t i = 0; i < desc->num_materials; i++)
        if (desc->materials[i].type != RT_DIELECTRIC && desc->materials[i].albedo.type == RT_IMAGE)
            out->has_image_textures = true;
    for (uint32_t i = 0; i < desc->num_materials; i++)
        if (desc->materials[i].type != RT_DIELECTRIC && desc->materials[i].albedo.type != RT_CONSTANT)
            out->has_textures = true;

    // images: RGB8, 3 bytes per texel (Texture.cuh:76); data == NULL means "no data" (Texture.cuh:83-84)
    size_t off = 0;
    for (uint32_t i = 0; i < desc->num_images; i++) {
        const rt_image_desc& im = desc->images[i];
        if (im.width < 0 || im.height < 0) {
            *err = "image " + std::to_string(i) + ": negative width or height";
            return RT_ERR_INVALID_SCENE;
        }
        const uint64_t texels = (uint64_t)im.width * (uint64_t)im.height;
        if (im.data && texels > (uint64_t)1 << 31) {  // the kernel indexes texel bytes with 64-bit offsets
            *err = "image " + std::to_string(i) + ": more than 2^31 texels";
            return RT_ERR_INVALID_SCENE;
        }
        const int bpt = g_texel_bytes == 4 ? 4 : 3;
        const size_t bytes = im.data ? (size_t)texels * (size_t)bpt : 0;
        if (bytes && off + bytes > (size_t)INT32_MAX) {  // imgs[] holds 32-bit byte offsets
            *err = "images exceed 2 GiB of texels in one scene";
            return RT_ERR_INVALID_SCENE;
        }
        out->imgs.push_back(bytes ? (int32_t)off : -1);
        out->imgs.push_back(im.width);
        out->imgs.push_back(im.height);
        out->imgs.push_back(bpt);
        // (each image is followed by at least 4 spare bytes: the kernels gather a texel as one dword, which for the
        // RGB8 layout's last texel reads one byte past it; then 16-B alignment)
        if (bytes && !with_texels) {
            off = (off + bytes + 4 + 15) & ~(size_t)15;
        } else if (bytes) {
            out->texels.resize(off + bytes);
            uint8_t* dst = out->texels.data() + off;
            if (bpt == 3) {
                std::memcpy(dst, im.data, bytes);
            } else {
                for (size_t t = 0; t < (size_t)texels; t++) {
                    dst[4 * t + 0] = im.data[3 * t + 0];
                    dst[4 * t + 1] = im.data[3 * t + 1];
                    dst[4 * t + 2] = im.data[3 * t + 2];
                    dst[4 * t + 3] = 0;
                }
            }
            off += bytes + 4;
            off = (off + 15) & ~(size_t)15;
            out->texels.resize(off, 0);
        }
    }

    Builder B;
    B.leaf_max = g_leaf_max;
    for (uint32_t i = 0; i < desc->num_hittables; i++) {
        const rt_hittable_desc& h = desc->hittables[i];
        if (!h.is_active) continue;  // thrust::remove_if of inactive objects (Hittable.cuh:311-312)
        if (h.type < RT_SPHERE || h.type > RT_YZRECT) {
            *err = "hittable " + std::to_string(i) + ": type " + std::to_string(h.type) + " invalid";
            return RT_ERR_INVALID_SCENE;
        }
        if (h.material < 0 || (uint32_t)h.material >= desc->num_materials) {
            *err = "hittable " + std::to_string(i) + ": material index " + std::to_string(h.material) +
                   " out of range";
            return RT_ERR_INVALID_SCENE;
        }
        // NaN or infinite geometry has no box (the reference's own AABB would poison every ancestor box)
        const bool sphere = h.type == RT_SPHERE;
        if (!std::isfinite(h.center[0]) || !std::isfinite(h.center[1]) || !std::isfinite(h.center[2]) ||
            (sphere ? !std::isfinite(h.radius) : (!std::isfinite(h.width) || !std::isfinite(h.height)))) {
            *err = "hittable " + std::to_string(i) + ": non-finite centre or size";
            return RT_ERR_INVALID_SCENE;
        }
        // A negative radius turns the reference's sphere box inside out (center - r > center + r,
        // Hittable.cuh:114), which its AABB test (AABB.cuh:30-50) never enters while Sphere::Hit still would: whether
        // the reference draws such a sphere depends on its tree shape.  The reference's editor keeps radii in
        // [0, FLT_MAX] (CudaLayer.cpp:496), so the library rejects the case instead of guessing.
        if (sphere && h.radius < 0.0f) {
            *err = "hittable " + std::to_string(i) + ": negative sphere radius";
            return RT_ERR_INVALID_SCENE;
        }
        out->has_rects = out->has_rects || !sphere;
        BuildPrim p;
        p.box = prim_box(h);
        for (int a = 0; a < 3; a++) p.centroid[a] = 0.5f * (p.box.lo[a] + p.box.hi[a]);
        p.src = (int)i;
        B.prims.push_back(p);
    }
    // the kernels address primitives as 32-B records at 32-bit byte offsets, and leaf references hold
    // first << 2 in a signed 32-bit value
    if (B.prims.size() >= ((size_t)1 << 26)) {
        *err = "more than 2^26 active primitives";
        return RT_ERR_INVALID_SCENE;
    }
    B.traversal = (float)g_sah_traversal_x10 / 10.0f;
    B.build_root();
    // Occupancy guard: a tree deeper than kOccupancyDepth costs the compact v3 kernel its 8th wave per SIMD (its
    // LDS stack grows by 128 B per level; C2's tree at depth 13 renders 8 % slower than at 12,
    // profiles/r02e_ab_sah.txt).  Dearer node visits make the SAH stop splitting earlier: retry with 1.5×, 2×,
    // 3× the cost and keep the first tree that fits; if none does, the first tree stays.
    if (B.max_depth > kOccupancyDepth && B.prims.size() > 1) {
        const float base = B.traversal;
        for (const float f : {1.5f, 2.0f, 3.0f}) {
            Builder T = B;
            T.traversal = base * f;
            T.build_root();
            if (T.max_depth <= kOccupancyDepth) {
                B = std::move(T);
                break;
            }
        }
        // still too deep (thousands of primitives): SAH splits under capacity limits that bound the depth — to
        // kOccupancyDepth when the primitives fit its leaves (8192 at leaf size 4: every 16-bit-reference scene),
        // else to one level above the shallowest tree that holds them (the LDS stack grows with the depth)
        uint32_t dmin = 1;
        while (((size_t)B.leaf_max << (dmin - 1)) < B.prims.size()) dmin++;
        const uint32_t target = std::max<uint32_t>(kOccupancyDepth, dmin + (dmin > kOccupancyDepth ? 1u : 0u));
        if (B.max_depth > target) {
            Builder T = B;
            T.traversal = base;
            T.depth_limit = target;
            T.build_root();
            B = std::move(T);
        }
    }
    out->num_prims = (uint32_t)B.prims.size();
    out->num_nodes = (uint32_t)B.nodes.size();
    out->depth = B.max_depth;

    out->nodes.resize((size_t)out->num_nodes * 16);
    // 16-bit references (internal nodes < 0x7fff, leaves ~(first << 2 | count - 1) with first < 8192) unless the
    // tree is too large: then 32-bit ones (the kernels' WIDE builds, render.hip RefW)
    out->wide_refs = !(out->num_nodes < 0x7fffu && out->num_prims < 8192u);
    out->nodes48.resize((size_t)out->num_nodes * 12);
    out->refs.resize((size_t)out->num_nodes * (out->wide_refs ? 2 : 1));
    for (uint32_t i = 0; i < out->num_nodes; i++) {
        pack_node16(B.nodes[i], out->nodes.data() + (size_t)i * 16);
        pack_node48(B.nodes[i], out->wide_refs, out->nodes48.data() + (size_t)i * 12);
        const Builder::Node& n = B.nodes[i];
        if (out->wide_refs) {
            out->refs[2 * (size_t)i] = (uint32_t)n.child[0];
            out->refs[2 * (size_t)i + 1] = (uint32_t)n.child[1];
        } else {
            out->refs[i] = ((uint32_t)n.child[0] & 0xffffu) | ((uint32_t)n.child[1] << 16);
        }
    }
    build_bounce_entries(B, out);
    // (at least one record: the BVH kernels' shade() loads record 0 for a miss before it knows the ray missed, so an
    // empty scene carries one zero record that no traversal reaches)
    out->prims.assign((size_t)std::max(out->num_prims, 1u) * 8, 0.0f);
    out->prim_source.resize(out->num_prims);
    for (uint32_t i = 0; i < out->num_prims; i++) {
        out->prim_source[i] = B.prims[B.order[i]].src;
        pack_prim(desc->hittables[out->prim_source[i]], out->prims.data() + (size_t)i * 8);
    }
    {  // the active rectangles in list order, and from them the sampled lights (build_light_table)
        std::vector<int> bvh_index(desc->num_hittables, -1);
        for (uint32_t i = 0; i < out->num_prims; i++) bvh_index[out->prim_source[i]] = (int)i;
        for (uint32_t i = 0; i < desc->num_hittables; i++) {
            const rt_hittable_desc& h = desc->hittables[i];
            if (bvh_index[i] < 0 || h.type == RT_SPHERE) continue;
            const float f[5] = {h.center[0], h.center[1], h.center[2], h.width, h.height};
            for (const float v : f) {
                uint32_t w;
                std::memcpy(&w, &v, 4);
                out->rects.push_back(w);
            }
            out->rects.push_back((uint32_t)bvh_index[i]);
            out->rects.push_back((uint32_t)h.material);
            out->rects.push_back(i);
        }
        build_light_table(out);
    }
    if (out->num_prims == 0) return RT_OK;
    // The reference's own BVH (its boxes and shape, Hittable.cuh:303-385) over the active primitives in list order.
    std::vector<int> objs;
    for (const BuildPrim& p : B.prims) objs.push_back(p.src);
    std::vector<RefNode> rn;
    build_reference_tree(desc->hittables, objs, 0, (int)objs.size(), 1, &rn);
    uint32_t rdepth = 0;
    for (const RefNode& n : rn) rdepth = std::max(rdepth, n.depth);
    // Every scene: the reference BVH with its primitive children as ~(BVH-order index) and, per BVH-order primitive,
    // its reference box — the BVH kernels' exactness check (render.hip bvh_clear): the rare rays whose closest hit the
    // reference's box culling or an exact tie could change replay the reference BVH over the BVH-order records.
    if (rdepth > kRefTreeMaxDepthBvh) {  // (2^26 primitives give <= 30: not reached within the primitive limit above)
        *err = "reference BVH deeper than " + std::to_string(kRefTreeMaxDepthBvh) + " levels";
        return RT_ERR_INVALID_SCENE;
    }
    {
        std::vector<int> bvh_index(desc->num_hittables, -1);
        for (uint32_t i = 0; i < out->num_prims; i++) bvh_index[out->prim_source[i]] = (int)i;
        out->bvh_boxes.resize((size_t)out->num_prims * 8);
        for (uint32_t i = 0; i < out->num_prims; i++)
            pack_ref_box(desc->hittables[out->prim_source[i]], out->bvh_boxes.data() + (size_t)i * 8);
        out->bvh_ref_nodes.resize(rn.size() * 8);
        for (size_t i = 0; i < rn.size(); i++) {
            float* o = out->bvh_ref_nodes.data() + i * 8;
            for (int k = 0; k < 2; k++) {
                const int c = rn[i].child[k];
                const int enc = c >= 0 ? c : ~bvh_index[~c];
                for (int a = 0; a < 3; a++) o[4 * k + a] = k == 0 ? rn[i].lo[a] : rn[i].hi[a];
                o[4 * k + 3] = bits_to_float((uint32_t)enc);
            }
        }
        // the same tree with each node's children's boxes in the node: (lo.xyz, ref), (hi.xyz, 0) per child, so the
        // replay tests both children of a node from one 64-B record and visits only the nodes whose box accepted
        out->bvh_ref_pairs.assign(rn.size() * 16, 0.0f);
        for (size_t i = 0; i < rn.size(); i++) {
            float* o = out->bvh_ref_pairs.data() + i * 16;
            for (int k = 0; k < 2; k++) {
                const int c = rn[i].child[k];
                const int enc = c >= 0 ? c : ~bvh_index[~c];
                if (c >= 0)
                    for (int a = 0; a < 3; a++) {
                        o[8 * k + a] = rn[c].lo[a];
                        o[8 * k + 4 + a] = rn[c].hi[a];
                    }
                o[8 * k + 3] = bits_to_float((uint32_t)enc);
            }
        }
    }
    // Small scenes: the primitives once more, in the order the reference's own BVH tests them (the flat kernel,
    // render.hip, tests every primitive of every ray in this order, so its closest hit breaks exact ties in t as
    // the reference's does)
    // together with the reference's own BVH (ref_nodes: its boxes and shape), which the flat kernel replays exactly
    // for the rare rays whose closest hit lies on a box face or ties (render.hip, ref_trace)
    if (out->num_prims <= kFlatMaxPrims) {
        if (rdepth <= kRefTreeMaxDepth) {
            std::vector<int> ord;
            reference_test_order(rn, 0, &ord);
            std::vector<int> flat_index(desc->num_hittables, -1);
            out->prims_flat.resize(ord.size() * 8);
            out->flat_boxes.resize(ord.size() * 8);
            out->flat_source.assign(ord.begin(), ord.end());
            for (size_t i = 0; i < ord.size(); i++) {
                flat_index[ord[i]] = (int)i;
                pack_prim(desc->hittables[ord[i]], out->prims_flat.data() + i * 8);
                pack_flat_box(desc->hittables[ord[i]], out->flat_boxes.data() + i * 8);
            }
            // the flat kernels scan one primitive type at a time (no per-primitive type branch): the reference test
            // order keeps each type contiguous (the tree splits at type-group boundaries, BVHNode's type sort); a
            // scene where it would not (never seen) simply does not get the flat kernels
            uint32_t runs[4][2] = {{0u, 0u}, {0u, 0u}, {0u, 0u}, {0u, 0u}};
            bool contiguous = true;
            for (size_t i = 0; i < ord.size();) {
                const int ty = desc->hittables[ord[i]].type;
                size_t j = i;
                while (j < ord.size() && desc->hittables[ord[j]].type == ty) j++;
                if (runs[ty][1] != 0u) contiguous = false;  // a second run of the same type
                runs[ty][0] = (uint32_t)i;
                runs[ty][1] = (uint32_t)j;
                i = j;
            }
            for (int ty = 0; ty < 4; ty++) {
                const uint32_t v = runs[ty][0] | (runs[ty][1] << 8);
                out->flat_runs[ty / 2] |= v << (16 * (ty % 2));
            }
            if (!contiguous) {
                out->prims_flat.clear();
                out->flat_boxes.clear();
                out->flat_source.clear();
                out->flat_runs[0] = out->flat_runs[1] = 0u;
                return RT_OK;
            }
            // per node: (lo.xyz, child 0) (hi.xyz, child 1); a primitive child is ~(its flat index)
            out->ref_nodes.resize(rn.size() * 8);
            for (size_t i = 0; i < rn.size(); i++) {
                float* o = out->ref_nodes.data() + i * 8;
                for (int k = 0; k < 2; k++) {
                    const int c = rn[i].child[k];
                    const int enc = c >= 0 ? c : ~flat_index[~c];
                    for (int a = 0; a < 3; a++) o[4 * k + a] = k == 0 ? rn[i].lo[a] : rn[i].hi[a];
                    o[4 * k + 3] = bits_to_float((uint32_t)enc);
                }
            }
            // ... and as child-pair records (bvh_ref_pairs' layout) for the wave-serial replay (ref_trace_wave)
            out->flat_ref_pairs.assign(rn.size() * 16, 0.0f);
            for (size_t i = 0; i < rn.size(); i++) {
                float* o = out->flat_ref_pairs.data() + i * 16;
                for (int k = 0; k < 2; k++) {
                    const int c = rn[i].child[k];
                    const int enc = c >= 0 ? c : ~flat_index[~c];
                    if (c >= 0)
                        for (int a = 0; a < 3; a++) {
                            o[8 * k + a] = rn[c].lo[a];
                            o[8 * k + 4 + a] = rn[c].hi[a];
                        }
                    o[8 * k + 3] = bits_to_float((uint32_t)enc);
                }
            }
        }
    }
    return RT_OK;
}

}  // namespace rt
