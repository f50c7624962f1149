// rt_tile_entry.h — per-tile entry records of the v3 kernels: the BVH leaves a tile's camera rays can reach.
//
// camera_ray (render.hip, Kernel.cu:139-146) is a pinhole: with A = k10_fwd − fov_fwd and the image-plane offset
// dist(u, v) = u·right + v·up, the point start + s·(second − start) is
//   origin + fov_fwd + s·A + (near + s·(far − near))·dist(u, v),
// which does not depend on (u, v) at s_e = −near / (far − near).  Every camera ray is therefore the half line
//   E + λ·D(u, v), λ ≥ −s_e,   E = origin + fov_fwd + s_e·A,   D(u, v) = A + (far − near)·dist(u, v),
// and, where s_e ≤ 0, lies in the forward nappe of the cone that E spans with the directions D of its tile.  D is affine
// in (u, v), so the tile's directions are a parallelogram and the nappe is the intersection of the four half spaces
// through E and two neighbouring corner directions.  A box that lies outside one of them (p-vertex test) holds nothing
// a camera ray of the tile can hit.  The beam is the tile's 8 × 8 pixels padded by one pixel on every side, which is
// three orders of magnitude above the binary32 rounding of the ray's own construction and of the tests below (each
// test also carries a relative slack of 2^-18 of its operands' magnitudes).
//
// One record per 8 × 8 tile, 16 B: eight 16-bit references.  Entry 0 = 0 (the root's index) is the marker "start at the
// root"; otherwise the entries are leaf references in the node tables' 16-bit form, ~(first << 2 | count − 1): within
// every leaf whose padded box meets the beam, each run of consecutive primitives that can meet it themselves (a sphere
// by its centre and radius, a rectangle by its extents) — a part of a leaf is walked like a leaf.  They come in
// traversal order, padded with the sentinel 0x7fff — entry 0 = 0x7fff: no candidate at all, the tile's camera rays miss.
// With TileFrame::occlusion the candidates that lie behind a sphere every ray of the beam hits are left out
// (tile_occlusion below): a tile inside a sphere's silhouette does not test the ground and the spheres behind it.
//
// The classifier is one host + device function, so that the pre-pass kernel and rt_tile_entries_host agree.
#pragma once

#include <cmath>
#include <cstdint>

#include "../../include/rt_hip.h"

#if defined(__HIPCC__)
#define RT_TILE_HD __host__ __device__
#else
#define RT_TILE_HD
#endif

namespace rt {

constexpr uint32_t kTileEntryMax = 8;          // K: references per record
constexpr uint32_t kTileEntryRoot = 0u;        // entry 0: start at the root
constexpr uint32_t kTileEntryNone = 0x7fffu;   // padding (the 16-bit sentinel)
constexpr uint32_t kTileEntryStack = 64;       // classifier stack (rt_render refuses deeper trees: kStackMax)

struct TileRecord {
    uint32_t w[4];  // entry i: bits 16·(i & 1) … of w[i / 2]
};

// The launch-uniform terms the classifier needs: KParams' camera fields and frame shape.
struct TileFrame {
    float origin[3], up[3], right[3], fov_fwd[3], k10_fwd[3];
    float near_plane, far_plane, width_f, cx, cy;
    uint32_t width, local_rows, band_rows, num_ranks, rank;
    uint32_t grid_w, grid_h;  // pixels rendered: x < grid_w, global row < grid_h (RT_FLAG_FAITHFUL_GRID)
    uint32_t tiles_x;
    uint32_t num_nodes, num_prims;
    uint32_t wide_refs;    // the scene's references need 32 bits: they do not fit the record
    uint32_t max_entries;  // at most kTileEntryMax; max_entries − 2 ≤ the kernel's stack entries
    uint32_t occlusion;    // drop candidates hidden behind a covering sphere (tile_occlusion, rt_set_tile_occlusion)
};

RT_TILE_HD inline TileRecord tile_record_root() {
    const uint32_t pad = kTileEntryNone | (kTileEntryNone << 16);
    return TileRecord{{kTileEntryRoot | (kTileEntryNone << 16), pad, pad, pad}};
}

RT_TILE_HD inline bool tile_finite(const float v) { return v - v == 0.0f; }

// Number of maximal runs of set bits in a run's 4-bit keep mask (its references), and the mask with the gap behind its
// first kept part filled (for a mask of two or more parts).
RT_TILE_HD inline uint32_t tile_mask_runs(const uint32_t m) {
    const uint32_t s = m & ~(m << 1);
    return (s & 1u) + (s >> 1 & 1u) + (s >> 2 & 1u) + (s >> 3 & 1u);
}
RT_TILE_HD inline uint32_t tile_mask_close_gap(uint32_t m) {
    uint32_t j = 0;
    while (j < 4u && !(m >> j & 1u)) j++;
    while (j < 4u && (m >> j & 1u)) j++;
    while (j < 4u && !(m >> j & 1u)) m |= 1u << j++;
    return m;
}

// A sphere record as the beam's apex E sees it (binary64): distance d of its centre, the cosine and sine of the angle θ
// between the centre's direction and the cone's axis, |radius|, and the shrunk and grown radii r_s < r < r_g that
// stand for Sphere::Hit's rounding (tile_occlusion).  False: a value is not finite, or d or the radius is 0 — such a
// sphere is left alone.
struct TileSphereView {
    double d, cos_t, sin_t, r, r_s, r_g, mag;
};
RT_TILE_HD inline bool tile_sphere_view(const float* p, const double E[3], const double axis[3], const double e_mag,
                                        const double s_far, TileSphereView& s) {
    if (!tile_finite(p[0]) || !tile_finite(p[1]) || !tile_finite(p[2]) || !tile_finite(p[3])) return false;
    const double v[3] = {(double)p[0] - E[0], (double)p[1] - E[1], (double)p[2] - E[2]};
    s.r = p[3] < 0.0f ? -(double)p[3] : (double)p[3];
    s.d = sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]);
    if (!(s.d > 0.0) || !(s.r > 0.0)) return false;
    s.cos_t = (v[0] * axis[0] + v[1] * axis[1] + v[2] * axis[2]) / s.d;
    const double s2 = 1.0 - s.cos_t * s.cos_t;
    s.sin_t = s2 > 0.0 ? sqrt(s2) : 0.0;
    const double c1 = (p[0] < 0.0f ? -(double)p[0] : (double)p[0]) + (p[1] < 0.0f ? -(double)p[1] : (double)p[1]) +
                      (p[2] < 0.0f ? -(double)p[2] : (double)p[2]);
    s.mag = e_mag + c1 + s.r + s_far;
    const double eps = 0x1p-18 * (s.mag * s.mag) / s.r;
    s.r_s = s.r - (0x1p-10 * s.r + eps);
    s.r_g = s.r + (0x1p-16 * s.r + eps);
    return s.r_g - s.r_g == 0.0;
}

// Occlusion culling of a tile's candidates (F.occlusion): clears in run_keep the primitives that lie, for every camera
// ray of the tile, behind a sphere that every camera ray of the tile hits.  In binary64 from the classifier's own E and
// corner directions, with + − × ÷ and sqrt alone, so host and device agree bit for bit.
//
// The beam lies in the circular cone about the axis a = Dc/|Dc| with half angle ρ, cos ρ = the smallest a·D_k/|D_k| of
// the four corners (a circular cone is convex, so it holds the parallelogram the corners span), 1 − cos ρ grown by
// 2^-8 of itself.  A ray of the beam at angle φ to the direction of a sphere's centre (distance d from E, radius r)
// enters the sphere at distance f(φ) = d cos φ − sqrt(r² − d² sin² φ) from E, which grows with φ where d > r; over the
// cone φ ranges within [max(0, θ − ρ), θ + ρ].
//
// Sphere::Hit in binary32 (v3_resolve_camera, the leaf loop) computes disc = b² − a·c from oc = o − centre with
// |oc| ≤ M = |E|₁ + |centre|₁ + r + s_far (s_far = −s_e·max|D_k|, the farthest ray start from E): b is off by at most
// 2^-22·M and disc by at most 2^-20·M² (three-term dot products of operands below M, the record's r² rounded once,
// a = |rd|² within 2^-22 of 1).  So the disc it sees is the exact one of a sphere of the same centre with a radius
// between r_s = r − (2^-10·r + eps) and r_g = r + (2^-16·r + eps), eps = 2^-18·M²/r: r_g² − r² and r² − r_s² are at
// least 2^-17·M², eight times the bound.  eps, not the relative term, is what dominates Sphere::Hit's error — for a
// sphere of radius 0.2 seen from 10 units in a scene of M = 25 it is 6 % of r, where 2^-10·r alone would be below the
// error of disc.  The relative terms stand above the rounding of the record's r and r²: 2^-10 on the occluder, whose
// shrinking only costs the tiles on its rim, 2^-16 (the classifier's own, prim_meets) on a primitive to be dropped —
// 2^-10 there would raise a ground sphere of radius 1000 by a whole unit and keep it in every tile.  The square root
// being monotonic, the near root Sphere::Hit computes lies between the exact entry distances of the grown and of the
// shrunk sphere, give or take b's 2^-22·M and the correctly rounded square root and division (2^-21·M together).  The rays' own rounding — a start within 2^-22·M of
// its place on the half line through E, a direction within 2^-23 — moves a centre by less than 2^-18·M ≤ eps as the
// ray sees it, and in angle by three orders of magnitude less than the pixel the beam is padded with (header).
//
// A (a sphere) covers the tile when r_s > 0, θ < 90°, cos(θ + ρ) > sqrt(1 − (r_s/d)²) — the cone lies inside the shrunk
// sphere's silhouette, so every ray has disc > 0 in binary32 too — and d − r_g > s_far + 16·kTmin + 2^-10·M: the entry
// root of every ray is above kTmin and is accepted.  Then every camera ray of the tile records a hit at or before
// T_A = f_{r_s}(θ + ρ) (+ 2^-21·M) from E.  B (a sphere) can only be entered at or after L_B = f_{r_g}(max(0, θ_B − ρ))
// (− 2^-21·M_B), and both of its roots lie there.  B is dropped where L_B > T_A·(1 + 2^-10) + 2^-18·(M_A + M_B) for
// the smallest T_A of the tile: along every ray A's accepted t is strictly below any t B could report (the same ray
// start is subtracted from both), so B never is the closest hit, never ties with it (kTieBit is set for a tie at the
// closest hit so far and is overwritten by a strictly closer acceptance — A's), and the hit record the scan or the leaf
// chain ends with — primitive, tag, t_best, tie bit — is the one it ends with when B is tested.  A itself is never
// dropped (L_A ≤ T_A).  Rectangles, unknown types and anything non-finite stay candidates and never occlude.
RT_TILE_HD inline void tile_occlusion(const float* prims, const float* E, const float (*D)[3], const float* Dc,
                                      const float s_e, const uint32_t* run_first, const uint32_t* run_count,
                                      uint32_t* run_keep, const uint32_t n_e) {
    if (n_e == 1 && run_count[0] == 1) return;
    const double Ed[3] = {(double)E[0], (double)E[1], (double)E[2]};
    double axis[3] = {(double)Dc[0], (double)Dc[1], (double)Dc[2]};
    const double alen = sqrt(axis[0] * axis[0] + axis[1] * axis[1] + axis[2] * axis[2]);
    if (!(alen > 0.0) || alen - alen != 0.0) return;
    for (int a = 0; a < 3; a++) axis[a] /= alen;
    double cos_rho = 1.0, dlen_max = 0.0;
    for (int k = 0; k < 4; k++) {
        const double x = D[k][0], y = D[k][1], z = D[k][2];
        const double len = sqrt(x * x + y * y + z * z);
        if (!(len > 0.0)) return;
        const double c = (x * axis[0] + y * axis[1] + z * axis[2]) / len;
        if (!(c <= 1.0)) return;  // (a NaN; c can only exceed 1 by rounding, which the slack below covers)
        if (c < cos_rho) cos_rho = c;
        if (len > dlen_max) dlen_max = len;
    }
    cos_rho = 1.0 - ((1.0 - cos_rho) * (1.0 + 0x1p-8) + 0x1p-44);
    if (!(cos_rho > 0.5)) return;
    const double sin_rho = sqrt(1.0 - cos_rho * cos_rho);
    const double s_far = -(double)s_e * dlen_max;
    const double e_mag = (Ed[0] < 0.0 ? -Ed[0] : Ed[0]) + (Ed[1] < 0.0 ? -Ed[1] : Ed[1]) + (Ed[2] < 0.0 ? -Ed[2] : Ed[2]);
    if (!(s_far >= 0.0) || s_far - s_far != 0.0 || e_mag - e_mag != 0.0) return;
    // per candidate L_B and M_B (L_B < 0: stays whatever covers the tile), and the covering sphere with the smallest T_A
    double lower[kTileEntryMax * 4], mags[kTileEntryMax * 4];
    double t_min = 0.0, mag_min = 0.0;
    uint32_t a_k = kTileEntryMax * 4, k = 0;
    for (uint32_t i = 0; i < n_e; i++)
        for (uint32_t j = 0; j < run_count[i]; j++, k++) {
            lower[k] = -1.0;
            mags[k] = 0.0;
            const float* p = prims + (size_t)(run_first[i] + j) * 8;
            uint32_t tag;
            __builtin_memcpy(&tag, p + 7, 4);
            TileSphereView s;
            if ((tag & 15u) != RT_SPHERE || !tile_sphere_view(p, Ed, axis, e_mag, s_far, s)) continue;
            const double rs = s.r_s, rg = s.r_g, dd = s.d * s.d, cc = s.cos_t * cos_rho, ss = s.sin_t * sin_rho;
            if (s.d > rg) {
                const double c = s.cos_t >= cos_rho ? 1.0 : cc + ss;  // cos(max(0, θ − ρ))
                const double s2 = 1.0 - c * c;
                const double q = rg * rg - dd * (s2 > 0.0 ? s2 : 0.0);
                // (q < 0: the cone passes the grown sphere by — it stays, as the classifier left it)
                if (q >= 0.0) {
                    lower[k] = s.d * c - sqrt(q);
                    mags[k] = s.mag;
                }
            }
            if (!(rs > 0.0) || !(s.cos_t > 0.0)) continue;
            if (!(s.d - rg > s_far + 0.016 + 0x1p-10 * s.mag)) continue;
            const double c = cc - ss;  // cos(θ + ρ), θ + ρ < 150°
            if (!(c > 0.0)) continue;
            const double q = rs * rs - dd * (1.0 - c * c);
            if (!(q > 0.0)) continue;
            const double T = s.d * c - sqrt(q);
            if (T - T != 0.0) continue;
            if (a_k == kTileEntryMax * 4 || T < t_min) {
                t_min = T;
                mag_min = s.mag;
                a_k = k;
            }
        }
    if (a_k == kTileEntryMax * 4) return;
    k = 0;
    for (uint32_t i = 0; i < n_e; i++)
        for (uint32_t j = 0; j < run_count[i]; j++, k++)
            if (k != a_k && lower[k] > t_min * (1.0 + 0x1p-10) + 0x1p-18 * (mag_min + mags[k])) run_keep[i] &= ~(1u << j);
}

// The record of tile `tile` (row-major in tiles_x) of the frame F over the 64-B node table `nodes` (rt_internal.h:
// per node the two children's boxes and their references as int32) and the 32-B primitive records `prims`.
RT_TILE_HD inline TileRecord tile_record(const float* nodes, const float* prims, const TileFrame& F, const uint32_t tile) {
    const TileRecord root = tile_record_root();
    if (F.num_nodes == 0 || F.wide_refs || F.tiles_x == 0 || F.band_rows == 0 || F.band_rows % 8u != 0) return root;
    if (F.max_entries < 1 || F.max_entries > kTileEntryMax) return root;
    const uint32_t bx = tile % F.tiles_x, by = tile / F.tiles_x;
    const uint32_t x0 = bx * 8u, ly0 = by * 8u;
    // partial tiles keep the root: their lanes outside the image render pixel 0's camera ray
    if (x0 + 8u > F.width || x0 + 8u > F.grid_w || ly0 + 8u > F.local_rows) return root;
    // (band_rows is a multiple of 8: the tile's rows lie in one band, global rows g0 … g0 + 7)
    const uint32_t band = ly0 / F.band_rows, within = ly0 - band * F.band_rows;
    const uint64_t g0l = ((uint64_t)band * F.num_ranks + F.rank) * F.band_rows + within;
    if (g0l + 8u > F.grid_h) return root;
    const float g0 = (float)(int)(uint32_t)g0l;
    const float near = F.near_plane, span = F.far_plane - F.near_plane;
    bool ok = tile_finite(near) && tile_finite(span) && span != 0.0f && tile_finite(F.width_f) && F.width_f > 0.0f &&
              tile_finite(F.cx) && tile_finite(F.cy);
    for (int a = 0; a < 3; a++)
        ok = ok && tile_finite(F.origin[a]) && tile_finite(F.up[a]) && tile_finite(F.right[a]) &&
             tile_finite(F.fov_fwd[a]) && tile_finite(F.k10_fwd[a]);
    if (!ok) return root;
    const float s_e = -near / span;
    if (!(s_e <= 0.0f) || !tile_finite(s_e)) return root;  // part of the ray would lie in the backward nappe
    // the beam's corners: pixel corners x0 − 1 … x0 + 9, global rows g0 − 1 … g0 + 9
    // (u = (x − cx + ξ) / width and v = (cy − g + ξ) / width with ξ in (0, 1])
    const float u_lo = ((float)(int)x0 - 1.0f - F.cx) / F.width_f, u_hi = ((float)(int)x0 + 9.0f - F.cx) / F.width_f;
    const float v_lo = (F.cy - (g0 + 8.0f)) / F.width_f, v_hi = (F.cy - g0 + 2.0f) / F.width_f;
    const float cu[4] = {u_lo, u_hi, u_hi, u_lo}, cv[4] = {v_lo, v_lo, v_hi, v_hi};
    float E[3], D[4][3], Dc[3], Dmax = 0.0f;
    for (int a = 0; a < 3; a++) {
        const float A = F.k10_fwd[a] - F.fov_fwd[a];
        E[a] = F.origin[a] + F.fov_fwd[a] + s_e * A;
        for (int k = 0; k < 4; k++) D[k][a] = A + span * (cu[k] * F.right[a] + cv[k] * F.up[a]);
        Dc[a] = 0.25f * ((D[0][a] + D[1][a]) + (D[2][a] + D[3][a]));
        ok = ok && tile_finite(E[a]);
    }
    // side planes through E, normals pointing into the beam and scaled to unit length
    float N[4][3];
    for (int k = 0; k < 4; k++) {
        const float* p = D[k];
        const float* q = D[(k + 1) & 3];
        float n[3] = {p[1] * q[2] - p[2] * q[1], p[2] * q[0] - p[0] * q[2], p[0] * q[1] - p[1] * q[0]};
        float len = 0.0f;
        for (int a = 0; a < 3; a++) len += n[a] * n[a];
        const float side = n[0] * Dc[0] + n[1] * Dc[1] + n[2] * Dc[2];
        if (!(len > 0.0f) || !tile_finite(len) || side == 0.0f) return root;
        const float inv = (side < 0.0f ? -1.0f : 1.0f) / sqrtf(len);
        for (int a = 0; a < 3; a++) N[k][a] = n[a] * inv;
        Dmax = fmaxf(Dmax, fmaxf(fabsf(p[0]), fmaxf(fabsf(p[1]), fabsf(p[2]))));
    }
    if (!ok || !tile_finite(Dmax)) return root;
    // a proper convex cone: every corner direction on the inner side of every plane
    for (int k = 0; k < 4; k++)
        for (int j = 0; j < 4; j++) {
            const float d = N[k][0] * D[j][0] + N[k][1] * D[j][1] + N[k][2] * D[j][2];
            if (!(d >= -0x1p-16f * Dmax)) return root;
        }
    // whether the box [lo, hi] (lo_x, hi_x, lo_y, hi_y, lo_z, hi_z) can meet the beam
    const auto meets = [&](const float lx, const float hx, const float ly, const float hy, const float lz,
                           const float hz) -> bool {
        for (int k = 0; k < 4; k++) {
            const float* n = N[k];
            const float px = n[0] >= 0.0f ? hx : lx, py = n[1] >= 0.0f ? hy : ly, pz = n[2] >= 0.0f ? hz : lz;
            const float d = n[0] * (px - E[0]) + n[1] * (py - E[1]) + n[2] * (pz - E[2]);
            const float mag = fabsf(n[0]) * (fabsf(px) + fabsf(E[0])) + fabsf(n[1]) * (fabsf(py) + fabsf(E[1])) +
                              fabsf(n[2]) * (fabsf(pz) + fabsf(E[2]));
            if (d < -0x1p-18f * mag) return false;  // (a NaN keeps the box)
        }
        return true;
    };
    // ... and a primitive record (rt_internal.h): a sphere by its centre's distance to the planes against its radius
    // (grown by 2^-16 of itself for the rounding of the record's r), a rectangle by its extents as a box
    const auto prim_meets = [&](const float* p) -> bool {
        uint32_t tag;
        __builtin_memcpy(&tag, p + 7, 4);
        const uint32_t type = tag & 15u;
        if (type == RT_SPHERE) {
            const float rad = fabsf(p[3]) * (1.0f + 0x1p-16f);
            for (int k = 0; k < 4; k++) {
                const float* n = N[k];
                const float d = n[0] * (p[0] - E[0]) + n[1] * (p[1] - E[1]) + n[2] * (p[2] - E[2]);
                const float mag = fabsf(n[0]) * (fabsf(p[0]) + fabsf(E[0])) + fabsf(n[1]) * (fabsf(p[1]) + fabsf(E[1])) +
                                  fabsf(n[2]) * (fabsf(p[2]) + fabsf(E[2]));
                if (d < -(rad + 0x1p-18f * mag)) return false;
            }
            return true;
        }
        // rectangle: p = (k, a0, a1, b0, b1, …); XY: (a, b, k) = (x, y, z), XZ: (x, z, y), YZ: (y, z, x)
        const float k0 = p[0] - 0.0001f - 0x1p-16f * fabsf(p[0]), k1 = p[0] + 0.0001f + 0x1p-16f * fabsf(p[0]);
        if (type == RT_XYRECT) return meets(p[1], p[2], p[3], p[4], k0, k1);
        if (type == RT_XZRECT) return meets(p[1], p[2], k0, k1, p[3], p[4]);
        if (type == RT_YZRECT) return meets(k0, k1, p[1], p[2], p[3], p[4]);
        return true;  // (an unknown type stays a candidate)
    };
    // the runs as they are found: first primitive, count (1 … 4) and, after tile_occlusion, which of them stay
    uint32_t run_first[kTileEntryMax], run_count[kTileEntryMax], run_keep[kTileEntryMax];
    uint32_t n_e = 0, sp = 0;
    int32_t stack[kTileEntryStack];
    int32_t node = 0;
    for (;;) {
        if ((uint32_t)node >= F.num_nodes) return root;  // (a malformed table)
        const float* r = nodes + (size_t)node * 16;
        int32_t c[2];
        __builtin_memcpy(&c[0], r + 12, 4);
        __builtin_memcpy(&c[1], r + 13, 4);
        const bool m[2] = {meets(r[0], r[1], r[2], r[3], r[8], r[9]), meets(r[4], r[5], r[6], r[7], r[10], r[11])};
        int32_t next = -1;  // (no internal child to continue with)
        for (int k = 0; k < 2; k++) {
            if (!m[k]) continue;
            if (c[k] < 0) {
                // the leaf's primitives one by one: each run of consecutive primitives that can meet the beam becomes
                // a reference of its own, ~(first << 2 | count − 1), which the leaf loop walks like a leaf
                const uint32_t l = ~(uint32_t)c[k], first = l >> 2, count = (l & 3u) + 1u;
                if (first + count > F.num_prims) return root;  // (a malformed table)
                uint32_t run = 0;
                for (uint32_t j = 0; j <= count; j++) {
                    if (j < count && prim_meets(prims + (size_t)(first + j) * 8)) {
                        run++;
                        continue;
                    }
                    if (run) {
                        if (n_e == F.max_entries) return root;
                        run_first[n_e] = first + j - run;
                        run_count[n_e] = run;
                        run_keep[n_e++] = (1u << run) - 1u;
                        run = 0;
                    }
                }
            } else if (next < 0) {
                next = c[k];
            } else {
                if (sp == kTileEntryStack) return root;
                stack[sp++] = c[k];
            }
        }
        if (next < 0) {
            if (sp == 0) break;
            next = stack[--sp];
        }
        node = next;
    }
    if (F.occlusion && n_e) tile_occlusion(prims, E, D, Dc, s_e, run_first, run_count, run_keep, n_e);
    // the kept primitives, run by run: a primitive dropped from the middle of a run splits it in two references.  The
    // record never holds more references than the n_e it holds without tile_occlusion (≤ F.max_entries): while it
    // would, a gap between two kept parts of a run is closed by putting its primitives back.
    uint32_t refs = 0;
    for (uint32_t i = 0; i < n_e; i++) refs += tile_mask_runs(run_keep[i]);
    for (uint32_t i = 0; i < n_e && refs > n_e; i++)
        while (refs > n_e && tile_mask_runs(run_keep[i]) > 1u) {
            run_keep[i] = tile_mask_close_gap(run_keep[i]);
            refs--;
        }
    uint32_t e[kTileEntryMax];
    for (uint32_t i = 0; i < kTileEntryMax; i++) e[i] = kTileEntryNone;
    uint32_t n_out = 0;
    for (uint32_t i = 0; i < n_e; i++) {
        uint32_t run = 0;
        for (uint32_t j = 0; j <= run_count[i]; j++) {
            if (j < run_count[i] && (run_keep[i] >> j & 1u)) {
                run++;
                continue;
            }
            if (run) {
                if (n_out == kTileEntryMax) return root;  // (cannot happen: refs ≤ n_e)
                e[n_out++] = ~(((run_first[i] + j - run) << 2) | (run - 1u)) & 0xffffu;
                run = 0;
            }
        }
    }
    return TileRecord{{e[0] | (e[1] << 16), e[2] | (e[3] << 16), e[4] | (e[5] << 16), e[6] | (e[7] << 16)}};
}

}  // namespace rt
