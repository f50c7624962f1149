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

}  // namespace rt
