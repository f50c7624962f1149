// rt_bounce_entry.h — where a bounce ray of the v3 kernels starts its traversal: at a leaf near its origin.
//
// For any leaf L of the BVH the tree is L plus the sibling subtrees S_a … S_1 that hang off L's ancestor path
// A_1 (the root) … A_a (L's parent): S_i is the child of A_i that is not on the path.  The siblings are packed two at a
// time, from the root, into extra node records behind the real ones ("chain nodes"): chain node (A_2k, side) holds S_2k
// and S_2k−1 as its children, their boxes copied from A_2k and A_2k−1, so leaves under a common ancestor share it.  An
// unpaired deepest sibling S_a (a odd) is referenced directly: a leaf reference is then tested without its box, an
// internal node visited without its own box test — both conservative.
//
// One 16-byte record per leaf, in the tile-entry record's form (rt_tile_entry.h): eight 16-bit references — the own leaf,
// then the chain from the deepest reference up, then kTileEntryNone as padding.  Entry 0 = kTileEntryRoot: start at the
// root (the chain needs more than seven references, or could outgrow the kernel's stack).  A ray that starts with entry
// 0 as its postponed leaf, entry 1 in `node` and the rest on its stack (deepest on top) walks the whole tree in the
// root traversal's order — own leaf, then the siblings from the deepest up — in ⌈a/2⌉ visits instead of a, with both
// box tests of every visit useful.
//
// Which leaf: a 3-D grid over the union of the boxes of the non-spanning primitives (a primitive spans when its box
// covers more than half of the scene's extent on two axes: a ground sphere), each cell holding the index of the record
// of the smallest leaf box that contains the cell's centre, else of the nearest one.  Origins outside the grid clamp to
// its border cells.  Any leaf's record covers the whole tree, so the choice changes the cost only, never the hit.
#pragma once

#include <cmath>
#include <cstdint>

#include "rt_tile_entry.h"

namespace rt {

constexpr uint32_t kBounceGridMaxCells = 4096;  // the grid is a uint16 per cell: 8 KB at most
constexpr uint32_t kBounceChainMax = 7;         // references behind the own leaf in a record

// The grid cell of the origin (x, y, z): per axis fma(o, inv, off) clamped to [0, dim − 1] (a NaN goes to 0), truncated.
// dimf = dim − 1 as floats.
RT_TILE_HD inline uint32_t bounce_cell(const float x, const float y, const float z, const float* inv, const float* off,
                                       const float* dimf, const uint32_t* dim) {
    const float fx = fminf(fmaxf(fmaf(x, inv[0], off[0]), 0.0f), dimf[0]);
    const float fy = fminf(fmaxf(fmaf(y, inv[1], off[1]), 0.0f), dimf[1]);
    const float fz = fminf(fmaxf(fmaf(z, inv[2], off[2]), 0.0f), dimf[2]);
    return ((uint32_t)fz * dim[1] + (uint32_t)fy) * dim[0] + (uint32_t)fx;
}

// ----- direction classes (rt_set_bounce_classes) ------------------------------------------------------------------
//
// A record's chain lists every sibling subtree of its leaf, but a ray that leaves the record's part of the grid in a
// known coarse direction cannot reach most of them.  Per record there are 25 records of the same form: one per
// direction class, holding the own leaf and only the siblings a ray of that class can reach from anywhere in the
// record's region, and record 24, today's full record, for every ray the argument below does not cover.
//
// Class: k = the axis of the largest |d| (a tie goes to the lower axis), the sign of d_k and the signs of the other
// two components: 8·k + (d_x < 0) + 2·(d_y < 0) + 4·(d_z < 0).  bounce_class() is the one function of host and kernel.
// It answers 24 when a component of d is zero, infinite or NaN (a rectangle test's acceptance of a NaN t does not
// depend on where the rectangle lies), and when the origin's unclamped cell coordinate is NaN, infinite or, summed
// over the axes, more than one cell outside the grid.
//
// Region R of a record: the box around the grid cells that name it, a cell being the origins whose exact
// o·inv + off falls in [i, i + 1); a border cell reaches one cell further outward, which is what bounce_class()
// admits.  A record no cell names, a "root" record and a scene with a flat grid axis (inv = 0) keep the full record
// in every class.
//
// Reachability of a sibling's box S (the box its parent node holds for it) from R in class (k, signs), in binary64
// with + − × and comparisons alone: with s = S.hi_k − R.lo_k for d_k > 0 (R.hi_k − S.lo_k for d_k < 0) a point of the
// ray o + t·d, t > 0, o in R, that lies in S has t·|d_k| ≤ s, and |t·d_j| ≤ t·|d_k| on the other axes, on d_j's
// side of o_j.  So S is unreachable when s < −m, or when on an axis j ≠ k its interval misses
// [R.lo_j, R.hi_j + s + m] (d_j > 0; [R.lo_j − s − m, R.hi_j] for d_j < 0) by more than m.
//
// The margin m = 2^-8·D + 2^-18·A, D = Σ_j (max(R.hi_j, S.hi_j) − min(R.lo_j, S.lo_j)), A = Σ_j max(|R.lo_j|, |R.hi_j|,
// |S.lo_j|, |S.hi_j|), is what makes "no point of the exact ray, t ≥ 0, lies within m of S on every axis" (what the
// test above establishes) imply "no binary32 test of a primitive in S accepts":
//   * the boxes: a primitive's box is its binary32 centre ± radius (or rectangle extent), rounded once, 2^-24 of the
//     coordinate; the carrier planes of nodes48 move outward only.  A cell's binary32 coordinate fma(o, inv, off)
//     differs from the exact o·inv + off by 2^-24 of itself, at most 2^-24·(dim + 2) cells ≤ 2^-16 of one cell for
//     dim ≤ 256, and R is at least one cell wide.  Both are below the second term and 2^-8 of the first.
//   * Sphere::Hit computes oc = o − c, a = d·d, b = oc·d, c' = oc·oc − r², disc = b² − a·c', every operation rounded
//     once (-ffp-contract=off), with |oc| ≤ D (o in R, the centre in S): |disc − exact| ≤ 40·2^-24·a·|oc|² <
//     2^-18.6·a·D², and exact disc = a·(r² − p²) for the line's distance p from the centre.  Where p ≥ r + m/2 the
//     exact disc is ≤ −a·m²/4 ≤ −2^-18·a·D²: the computed one is negative and the test rejects.  Where p < r + m/2 the
//     line's closest point to the centre lies within m/2 of the sphere, so of S, and o lies m or more from S: that
//     point is at t ≤ −(m/2)/|d| ≤ −2^-9·D/|d|.  The computed roots are −b/a ± sqrt(disc)/a with b/a within 2^-21·D/|d|
//     of that t and, the exact disc being ≤ 0 or its roots themselves points of S behind o, sqrt(disc)/a either below
//     sqrt(2^-18.6)·D/|d| = 2^-9.3·D/|d| or leading to roots ≤ −m/|d|: both roots are negative, below kTmin.
//   * a rectangle's t = (k − o_k)/d_k has the exact sign (a correctly rounded quotient of a difference of exact sign),
//     so a plane behind the ray is rejected by t < kTmin; in front, its in-plane point o + t·d is off by 3·2^-24 of
//     its terms' magnitudes, below 4·A wherever the point is within A of the rectangle: less than the second term.
// A test that does not accept leaves the hit record alone: a dropped primitive is neither the closest hit nor ties
// with it (kTieBit is set by an accepted t equal to the closest so far), at any t > kTmin.
//
// A sibling that holds a spanning primitive is never dropped (the grid is built over the others, so its box says
// nothing about R).  Two forms: 1 keeps a chain node of today's table when either of its children is reachable;
// 2 pairs the reachable siblings anew, from the root, as chain nodes behind today's (equal pairs stored once).
constexpr uint32_t kBounceClasses = 25;    // records per leaf in the class table
constexpr uint32_t kBounceClassFull = 24;  // ... of which this one is the leaf's full record

// (dx, dy, dz): the ray's direction; (ex, ey, ez): per axis the cell coordinate u = fma(o, inv, off) minus u clamped to
// the grid, [0, dim]: how far outside the grid the origin lies, in cells.
RT_TILE_HD inline uint32_t bounce_class(const float dx, const float dy, const float dz, const float ex, const float ey,
                                        const float ez) {
    const float ax = fabsf(dx), ay = fabsf(dy), az = fabsf(dz);
    const uint32_t k = ax >= ay ? (ax >= az ? 0u : 2u) : (ay >= az ? 1u : 2u);
    uint32_t bx, by, bz;
    __builtin_memcpy(&bx, &dx, 4);
    __builtin_memcpy(&by, &dy, 4);
    __builtin_memcpy(&bz, &dz, 4);
    const uint32_t cls = k * 8u + ((bx >> 31) | (by >> 31) << 1 | (bz >> 31) << 2);
    // (a NaN fails each comparison: the sums carry it where fminf would drop it)
    const bool ok = fminf(fminf(ax, ay), az) > 0.0f && (ax + ay) + az < INFINITY && (fabsf(ex) + fabsf(ey)) + fabsf(ez) <= 1.0f;
    return ok ? cls : kBounceClassFull;
}

// The same from an origin and the grid, as the kernel forms ex, ey, ez (dims = dim as floats).
RT_TILE_HD inline uint32_t bounce_class_at(const float* o, const float* d, const float* inv, const float* off,
                                           const float* dims) {
    float e[3];
    for (int i = 0; i < 3; i++) {
        const float u = fmaf(o[i], inv[i], off[i]);
        e[i] = u - fminf(fmaxf(u, 0.0f), dims[i]);
    }
    return bounce_class(d[0], d[1], d[2], e[0], e[1], e[2]);
}

}  // namespace rt
