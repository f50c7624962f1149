"""CPU tests of the v3 kernels' bounce entries (csrc/rt_bounce_entry.h, built by scene_build.cpp and read here through
rt_bounce_entries_host / rt_bounce_entry_cells): chain nodes behind the real BVH nodes, one record per leaf, and the
origin grid that names a record for a ray origin.

What must hold for every scene: each record covers the whole tree (it reaches every leaf exactly once), the chain
nodes' boxes are the sibling boxes they copy (bit-equal before the references are packed into their low bytes, moved
outward only after), no record can outgrow the kernel's `depth` stack entries, every grid cell names a record, and a
traversal started from the record an origin looks up returns the brute-force closest hit — with no tolerance: both
sides run the same primitive tests (binary64 here, on the binary32 tables), so they answer the same question, and the
boxes only cull.
"""
from __future__ import annotations

import collections
import ctypes as C
import functools

import numpy as np
import pytest

from adversarial_scene import adversarial_scene_tiled
from cudaraytracer_amd import abi, scenes
from cudaraytracer_amd._lib import lib

ROOT_MARK, NONE, LEAF = 0, 0x7FFF, 0x8000
T_MIN = 0.001
SLACK = 1.0 + 2.0 ** -20  # render.hip kSlabSlack
RAYS = 3000


def _spheres(items):
    m = (abi.MaterialDesc * 1)()
    m[0].type, m[0].albedo.type, m[0].albedo.image = abi.RT_LAMBERTIAN, abi.RT_CONSTANT, -1
    m[0].albedo.color[:] = (0.5, 0.5, 0.5)
    h = (abi.HittableDesc * len(items))()
    for k, (c, r) in enumerate(items):
        h[k].type, h[k].is_active, h[k].radius, h[k].material = abi.RT_SPHERE, 1, r, 0
        h[k].center[:] = c
    return scenes.Scene(h, m, [])


_ENDS = [((0.0, -1000.0, 0.0), 1000.0), ((-4.0, 1.0, 0.0), 1.0), ((4.0, 1.0, 0.0), 1.0), ((0.0, 1.0, 0.0), 1.0),
         ((2.0, 1.0, 2.5), 1.0)]  # tests/test_gpu_path_end.py's five-primitive scene (its geometry)
_SCENES = {
    "one": lambda: _spheres([((0.5, 1.0, -2.0), 1.0)]),
    "two": lambda: _spheres([((0.0, 0.0, 0.0), 1.0), ((3.0, 0.5, 0.0), 0.5)]),
    "ends": lambda: _spheres(_ENDS),
    "rtiow": lambda: scenes.builtin(scenes.SCENE_RTIOW),
    "touching": adversarial_scene_tiled,
    "cornell": lambda: scenes.builtin(scenes.SCENE_CORNELL),
    "field": lambda: scenes.sphere_field(3000, 5),
}
TABLE_SCENES = sorted(_SCENES)

Tables = collections.namedtuple("Tables", "info nodes prims chain nodes48 refs records grid")


@functools.lru_cache(maxsize=None)
def tables(key) -> Tables:
    sc = _SCENES[key]() if key in _SCENES else key
    d = sc.desc()
    L = lib()
    hi = abi.HostTablesInfo()
    assert L.rt_build_host_tables(C.byref(d), None, None, None, None, C.byref(hi)) == 0
    nodes = np.zeros((max(1, hi.num_nodes), 16), np.float32)
    prims = np.zeros((max(1, hi.num_prims), 8), np.float32)
    mats = np.zeros((max(1, hi.num_materials), 12), np.float32)
    src = np.zeros(max(1, hi.num_prims), np.int32)
    fp = lambda a: a.ctypes.data_as(C.POINTER(C.c_float))
    assert L.rt_build_host_tables(C.byref(d), fp(nodes), fp(prims), fp(mats), src.ctypes.data_as(C.POINTER(C.c_int32)),
                                  C.byref(hi)) == 0
    info = abi.BounceEntriesInfo()
    assert L.rt_bounce_entries_host(C.byref(d), None, None, None, None, None, C.byref(info)) == 0, L.rt_last_error()
    assert info.num_nodes == hi.num_nodes and info.depth == hi.depth
    total = info.num_nodes + info.num_chain_nodes
    chain = np.zeros((max(1, info.num_chain_nodes), 16), np.float32)
    nodes48 = np.zeros((max(1, total), 12), np.float32)
    refs = np.zeros(max(1, total), np.uint32)
    rec = np.zeros((max(1, info.num_records), 4), np.uint32)
    grid = np.zeros(max(1, info.grid_dim[0] * info.grid_dim[1] * info.grid_dim[2]), np.uint16)
    if info.num_records:
        assert L.rt_bounce_entries_host(C.byref(d), fp(chain), fp(nodes48), refs.ctypes.data_as(C.POINTER(C.c_uint32)),
                                        rec.ctypes.data_as(C.POINTER(C.c_uint32)),
                                        grid.ctypes.data_as(C.POINTER(C.c_uint16)), C.byref(info)) == 0
    records = np.stack([rec & 0xFFFF, rec >> 16], axis=2).reshape(-1, 8).astype(np.int64)
    for a in (nodes, prims, chain, nodes48, refs, records, grid):
        a.setflags(write=False)
    return Tables(info, nodes[: hi.num_nodes], prims[: hi.num_prims], chain[: info.num_chain_nodes], nodes48[:total],
                  refs[:total], records[: info.num_records], grid)


def children(T: Tables, n: int):
    return int(T.refs[n]) & 0xFFFF, int(T.refs[n]) >> 16


def leaves_under(T: Tables, ref: int):
    """Leaf references below `ref` (a node index, real or chain, or a leaf reference), with repetitions."""
    out, todo = [], [ref]
    while todo:
        r = todo.pop()
        if r >= LEAF:
            out.append(r)
        else:
            assert r < len(T.refs), f"reference {r} names no node"
            todo.extend(children(T, r))
    return out


@pytest.mark.parametrize("key", TABLE_SCENES)
def test_every_record_reaches_every_leaf_exactly_once(key):
    T = tables(key)
    assert T.info.num_records > 0 and T.info.num_nodes + T.info.num_chain_nodes < 0x7FFF
    whole = collections.Counter(leaves_under(T, 0))
    assert len(T.records) == sum(whole.values())  # one record per leaf of the tree
    if len(T.prims) > 1:
        assert set(whole.values()) == {1}
    started = 0
    for e in T.records:
        if e[0] == ROOT_MARK:
            assert np.all(e[1:] == NONE)
            continue
        started += 1
        assert e[0] >= LEAF and e[1] != NONE
        used = e[e != NONE]
        assert np.all(e[len(used):] == NONE), "the references are packed from the front"
        got = collections.Counter()
        for r in used:
            got.update(leaves_under(T, int(r)))
        assert got == whole
        # behind the leaf: at most one direct reference (a real node or a leaf), then chain nodes only
        assert all(int(r) >= T.info.num_nodes and int(r) < LEAF for r in used[2:])
    assert started > 0, "no record starts anywhere but the root"
    # the real nodes' child references do not reach the chain nodes
    for n in range(T.info.num_nodes):
        assert all(c >= LEAF or c < T.info.num_nodes for c in children(T, n))


@pytest.mark.parametrize("key", TABLE_SCENES)
def test_chain_boxes_are_the_sibling_boxes(key):
    T = tables(key)
    N = T.info.num_nodes
    box_of = {}  # child reference (32-bit) -> the six planes its parent holds for it
    for n in range(N):
        r = T.nodes[n]
        c = r[12:14].view(np.int32)
        box_of.setdefault(int(c[0]), []).append(np.array([r[0], r[1], r[2], r[3], r[8], r[9]], np.float32))
        box_of.setdefault(int(c[1]), []).append(np.array([r[4], r[5], r[6], r[7], r[10], r[11]], np.float32))
    assert len(T.chain) > 0 or len(T.prims) <= 2
    for k in range(len(T.chain)):
        r, p = T.chain[k], T.nodes48[N + k]
        c = r[12:14].view(np.int32)
        raw = [np.array([r[0], r[1], r[2], r[3], r[8], r[9]], np.float32),
               np.array([r[4], r[5], r[6], r[7], r[10], r[11]], np.float32)]
        packed = [np.array([p[0], p[1], p[2], p[3], p[8], p[9]], np.float32),
                  np.array([p[4], p[5], p[6], p[7], p[10], p[11]], np.float32)]
        for s in range(2):
            assert any(np.array_equal(raw[s].view(np.uint32), b.view(np.uint32)) for b in box_of[int(c[s])])
            lo, hi = packed[s][0::2], packed[s][1::2]
            assert np.all(lo <= raw[s][0::2]) and np.all(hi >= raw[s][1::2])
            assert np.array_equal(packed[s][2:].view(np.uint32), raw[s][2:].view(np.uint32))  # y and z planes: as they were
            ref16 = int(c[s]) & 0xFFFF
            bits = packed[s][:2].view(np.uint32)
            assert (int(bits[0]) & 0xFF) | ((int(bits[1]) & 0xFF) << 8) == ref16 == children(T, N + k)[s]
            # < 512 ulps outward
            assert np.all(np.abs(packed[s][:2].view(np.int32).astype(np.int64) - raw[s][:2].view(np.int32)) < 512) or \
                np.any(raw[s][:2] == 0.0)


def _height(T: Tables, ref: int, memo) -> int:
    """Internal levels below and including `ref` (0 for a leaf)."""
    if ref >= LEAF:
        return 0
    if ref not in memo:
        memo[ref] = 1 + max(_height(T, c, memo) for c in children(T, ref))
    return memo[ref]


@pytest.mark.parametrize("key", TABLE_SCENES)
def test_no_record_outgrows_the_stack(key):
    """Every box test hits and either child may be the near one: a visit with h entries below writes entry h, its near
    child is visited with h + 1 below, its far one with h.  The kernel's stack holds `depth` entries."""
    T = tables(key)
    memo = {}
    depth = T.info.depth
    assert _height(T, 0, memo) <= depth  # (the root traversal's own bound)
    for e in T.records:
        if e[0] == ROOT_MARK:
            continue
        used = [int(r) for r in e[1:] if r != NONE]
        m = len(used)
        assert m - 1 <= depth
        for j, r in enumerate(used):
            h = m - 1 - j
            if r >= LEAF:
                continue
            if r >= T.info.num_nodes:  # a chain node: its own box tests, then a child one entry higher
                top = h + 1 + max(_height(T, c, memo) for c in children(T, r))
            else:
                top = h + _height(T, r, memo)
            assert top <= depth, (e.tolist(), j, top, depth)


@pytest.mark.parametrize("key", TABLE_SCENES)
def test_grid_cells_name_records_and_origins_clamp(key):
    T = tables(key)
    dim = np.array(list(T.info.grid_dim), np.int64)
    assert np.all(dim >= 1) and 1 <= dim.prod() <= 4096 and len(T.grid) == dim.prod()
    assert np.all(T.grid < T.info.num_records)
    org = np.array(list(T.info.grid_origin), np.float64)
    inv = np.array(list(T.info.grid_inv), np.float64)
    ext = np.where(inv > 0, dim / np.where(inv > 0, inv, 1.0), 0.0)
    centre = org + 0.5 * ext
    far = 10.0 * (ext.max() + 1.0)
    pts, want = [], []
    for sx in (-1, 0, 1):
        for sy in (-1, 0, 1):
            for sz in (-1, 0, 1):
                s = np.array([sx, sy, sz])
                pts.append(centre + s * far)
                ijk = np.where(s < 0, 0, np.where(s > 0, dim - 1, np.minimum((dim * 0.5).astype(np.int64), dim - 1)))
                ijk = np.where(inv > 0, ijk, 0)
                want.append((ijk[2] * dim[1] + ijk[1]) * dim[0] + ijk[0])
    pts += [np.array([np.nan, np.inf, -np.inf]), np.array([3e38, -3e38, 0.0])]
    o = np.array(pts, np.float32)
    cells = np.zeros(len(o), np.uint32)
    assert lib().rt_bounce_entry_cells(C.byref(T.info), o.ctypes.data_as(C.POINTER(C.c_float)), len(o),
                                       cells.ctypes.data_as(C.POINTER(C.c_uint32))) == 0
    assert np.all(cells < dim.prod())
    got, want = cells[: len(want)].astype(np.int64), np.array(want, np.int64)
    odd = dim % 2 == 1  # an even axis has the centre on a cell border: only the clamped axes are compared there
    for k in range(len(want)):
        g = np.array([got[k] % dim[0], got[k] // dim[0] % dim[1], got[k] // (dim[0] * dim[1])])
        w = np.array([want[k] % dim[0], want[k] // dim[0] % dim[1], want[k] // (dim[0] * dim[1])])
        s = np.array([(k // 9) - 1, (k // 3) % 3 - 1, k % 3 - 1])
        cmp = (s != 0) | odd | (inv <= 0)
        assert np.array_equal(g[cmp], w[cmp]), (k, g, w)


def test_scene_beyond_16_bit_references_has_no_table():
    sc = scenes.sphere_field(9000, 6)
    d = sc.desc()
    info = abi.BounceEntriesInfo()
    assert lib().rt_bounce_entries_host(C.byref(d), None, None, None, None, None, C.byref(info)) == 0
    assert info.num_records == 0 and info.num_chain_nodes == 0 and info.num_nodes > 0
    assert tuple(info.grid_dim) == (0, 0, 0)
    o = np.zeros(3, np.float32)
    cell = np.zeros(1, np.uint32)
    assert lib().rt_bounce_entry_cells(C.byref(info), o.ctypes.data_as(C.POINTER(C.c_float)), 1,
                                       cell.ctypes.data_as(C.POINTER(C.c_uint32))) < 0


def test_field_scene_is_depth_limited():
    T = tables("field")
    assert len(T.prims) == 3001 and T.info.depth == 12 and T.info.num_chain_nodes > 0


# ----- closest hits ---------------------------------------------------------------------------------------------

def _prim_t(P, o, d, t_best):
    """The primitive tests of render.hip's leaf loop on records P (R, 8) for rays (o, d) (R, 3), binary64: the accepted
    t per ray, inf where the test rejects.  t_best (R,) is the closest hit so far."""
    tag = P[:, 7].astype(np.float32).view(np.uint32) & 15
    t = np.full(len(o), np.inf)
    sph = tag == abi.RT_SPHERE
    with np.errstate(all="ignore"):
        oc = o - P[:, 0:3]
        a = np.einsum("ij,ij->i", d, d)
        b = np.einsum("ij,ij->i", oc, d)
        c = np.einsum("ij,ij->i", oc, oc) - P[:, 4]
        disc = b * b - a * c
        sq = np.sqrt(np.where(disc > 0, disc, 0.0))
        t1, t2 = (-b - sq) / a, (-b + sq) / a
        ok1 = (t1 < t_best) & (t1 > T_MIN)
        ok2 = (t2 < t_best) & (t2 > T_MIN)
        ts = np.where(ok1, t1, np.where(ok2, t2, np.inf))
        t = np.where(sph & (disc > 0), ts, t)
        for ty, (ik, ia, ib) in ((abi.RT_XYRECT, (2, 0, 1)), (abi.RT_XZRECT, (1, 0, 2)), (abi.RT_YZRECT, (0, 1, 2))):
            m = tag == ty
            if not m.any():
                continue
            tr = (P[:, 0] - o[:, ik]) / d[:, ik]
            xx, yy = o[:, ia] + tr * d[:, ia], o[:, ib] + tr * d[:, ib]
            ok = ~((tr < T_MIN) | (tr > t_best)) & ~((xx < P[:, 1]) | (xx > P[:, 2]) | (yy < P[:, 3]) | (yy > P[:, 4]))
            t = np.where(m, np.where(ok, tr, np.inf), t)
    return t


def brute_force(T: Tables, o, d):
    best = np.full(len(o), np.inf)
    P = T.prims.astype(np.float64)
    for k in range(len(P)):
        t = _prim_t(np.broadcast_to(P[k], (len(o), 8)), o, d, best)
        best = np.minimum(best, t)
    return best


def traverse(T: Tables, o, d, start):
    """Closest hits of the rays by a stack traversal of the 48-byte table: ray r starts from the references start[r]
    (the first is visited first).  Returns (t, node visits per ray)."""
    R = len(o)
    B = T.nodes48.astype(np.float64)
    P = T.prims.astype(np.float64)
    ch = np.stack([T.refs & 0xFFFF, T.refs >> 16], axis=1).astype(np.int64)
    cap = T.info.depth + 12
    stack = np.full((R, cap), NONE, np.int64)
    sp = np.zeros(R, np.int64)
    for r in range(R):
        s = [int(x) for x in start[r]][::-1]
        stack[r, : len(s)] = s
        sp[r] = len(s)
    best = np.full(R, np.inf)
    visits = np.zeros(R, np.int64)
    with np.errstate(all="ignore"):
        inv = np.clip(1.0 / d, -1e20, 1e20)
    rows = np.arange(R)
    cur = np.full(R, NONE, np.int64)

    def pop(mask):
        has = mask & (sp > 0)
        sp[has] -= 1
        cur[mask] = NONE
        cur[has] = stack[rows[has], sp[has]]

    pop(np.ones(R, bool))
    while True:
        leaf = cur >= LEAF
        node = cur < NONE
        if not (leaf.any() or node.any()):
            break
        if leaf.any():
            idx = np.nonzero(leaf)[0]
            l = cur[idx] ^ 0xFFFF
            first, count = l >> 2, (l & 3) + 1
            for j in range(4):
                m = count > j
                if not m.any():
                    break
                ii = idx[m]
                t = _prim_t(P[first[m] + j], o[ii], d[ii], best[ii])
                best[ii] = np.minimum(best[ii], t)
            pop(leaf)
        if node.any():
            idx = np.nonzero(node)[0]
            visits[idx] += 1
            n = cur[idx]
            b = B[n]
            oo, ii = o[idx], inv[idx]
            hit, tmin = [], []
            for cix, (x0, x1, y0, y1, z0, z1) in enumerate(((0, 1, 2, 3, 8, 9), (4, 5, 6, 7, 10, 11))):
                with np.errstate(all="ignore"):
                    tx0, tx1 = (b[:, x0] - oo[:, 0]) * ii[:, 0], (b[:, x1] - oo[:, 0]) * ii[:, 0]
                    ty0, ty1 = (b[:, y0] - oo[:, 1]) * ii[:, 1], (b[:, y1] - oo[:, 1]) * ii[:, 1]
                    tz0, tz1 = (b[:, z0] - oo[:, 2]) * ii[:, 2], (b[:, z1] - oo[:, 2]) * ii[:, 2]
                    near = np.fmax(np.fmax(np.fmin(tx0, tx1), np.fmin(ty0, ty1)), np.fmax(np.fmin(tz0, tz1), T_MIN))
                    far = np.fmin(np.fmin(np.fmax(tx0, tx1), np.fmax(ty0, ty1)), np.fmin(np.fmax(tz0, tz1), best[idx]))
                    far = far * SLACK
                hit.append(near <= far)
                tmin.append(near)
            both = hit[0] & hit[1]
            swap = tmin[1] < tmin[0]
            c0, c1 = ch[n, 0], ch[n, 1]
            nearc = np.where(both, np.where(swap, c1, c0), np.where(hit[0], c0, c1))
            farc = np.where(swap, c0, c1)
            push = idx[both]
            assert np.all(sp[push] < cap)
            stack[push, sp[push]] = farc[both]
            sp[push] += 1
            anyh = hit[0] | hit[1]
            cur[idx[anyh]] = nearc[anyh]
            none = np.zeros(R, bool)
            none[idx[~anyh]] = True
            pop(none)
    return best, visits


def _rays(T: Tables, seed: int):
    rng = np.random.default_rng(seed)
    P = T.prims.astype(np.float64)
    tag = T.prims[:, 7].view(np.uint32) & 15
    n = RAYS // 3

    def unit(k):
        v = rng.normal(size=(k, 3))
        return v / np.linalg.norm(v, axis=1)[:, None]

    def on_prims(which):
        out = np.zeros((len(which), 3))
        for r, k in enumerate(which):
            p = P[k]
            if tag[k] == abi.RT_SPHERE:
                out[r] = p[0:3] + p[3] * unit(1)[0]
            else:
                ik, ia, ib = {abi.RT_XYRECT: (2, 0, 1), abi.RT_XZRECT: (1, 0, 2), abi.RT_YZRECT: (0, 1, 2)}[int(tag[k])]
                out[r, ik] = p[0]
                out[r, ia] = rng.uniform(p[1], p[2])
                out[r, ib] = rng.uniform(p[3], p[4])
        return out

    org = np.array(list(T.info.grid_origin), np.float64)
    inv = np.array(list(T.info.grid_inv), np.float64)
    dim = np.array(list(T.info.grid_dim), np.float64)
    ext = np.where(inv > 0, dim / np.where(inv > 0, inv, 1.0), 0.0)
    surface = on_prims(rng.integers(0, len(P), n))
    # the ground: the largest primitive's surface towards points of the grid's volume (a sphere: the part of it that
    # faces the others; a rectangle: its own area)
    size = np.where(tag == abi.RT_SPHERE, np.abs(P[:, 3]), np.maximum(P[:, 2] - P[:, 1], P[:, 4] - P[:, 3]))
    g = int(np.argmax(size))
    if tag[g] == abi.RT_SPHERE:
        q = org + rng.uniform(size=(n, 3)) * ext - P[g, 0:3]
        ground = P[g, 0:3] + P[g, 3] * q / np.linalg.norm(q, axis=1)[:, None]
    else:
        ground = on_prims(np.full(n, g))
    anywhere = org - 0.25 * ext - 0.5 + rng.uniform(size=(RAYS - 2 * n, 3)) * (1.5 * ext + 1.0)
    o = np.concatenate([surface, ground, anywhere]).astype(np.float32).astype(np.float64)
    d = unit(len(o)).astype(np.float32).astype(np.float64)
    return o, d


@pytest.mark.parametrize("key", TABLE_SCENES)
def test_traversal_from_the_looked_up_record_finds_the_closest_hit(key):
    T = tables(key)
    o, d = _rays(T, 11)
    o32 = np.ascontiguousarray(o, np.float32)
    cells = np.zeros(len(o), np.uint32)
    assert lib().rt_bounce_entry_cells(C.byref(T.info), o32.ctypes.data_as(C.POINTER(C.c_float)), len(o),
                                       cells.ctypes.data_as(C.POINTER(C.c_uint32))) == 0
    rec = T.records[T.grid[cells]]
    start = [[0] if e[0] == ROOT_MARK else [int(r) for r in e if r != NONE] for e in rec]
    want = brute_force(T, o, d)
    got, visits = traverse(T, o, d, start)
    root, root_visits = traverse(T, o, d, [[0]] * len(o))
    hits = np.isfinite(want)
    print(f"{key}: {len(o)} rays, {hits.sum()} hit, {sum(len(s) > 1 for s in start)} start at a leaf; node visits per "
          f"ray {visits.mean():.2f} from the records, {root_visits.mean():.2f} from the root")
    assert np.array_equal(root, want)  # (the traversal itself, on the real nodes alone)
    bad = np.nonzero(got != want)[0]
    assert len(bad) == 0, (len(bad), bad[:5].tolist(), got[bad[:5]].tolist(), want[bad[:5]].tolist())
    assert 0 < hits.sum() < len(o) or key in ("cornell",)


def test_switch():
    L = lib()
    assert L.rt_set_bounce_entries(0) == 1
    assert L.rt_set_bounce_entries(1) == 0
    for bad in (-1, 2, 1 << 20):
        assert L.rt_set_bounce_entries(bad) < 0
        assert b"rt_set_bounce_entries" in L.rt_last_error()
    assert L.rt_set_bounce_entries(1) == 1  # (a refused value changes nothing)
