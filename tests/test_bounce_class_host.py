"""CPU tests of the direction classes of the v3 kernels' bounce entries (csrc/rt_bounce_entry.h, built by
scene_build.cpp, read here through rt_bounce_class_entries_host): per leaf record 25 records, one per class of ray
direction, which list only the sibling subtrees a ray of the class can reach from the record's region of the origin
grid, and the full record as class 24.

What must hold for every scene and both forms: class 24 is the full record bit for bit; a class record holds the own
leaf first and a subset of the full record's siblings, each once; every sibling it leaves out fails the header's box
test, recomputed here in numpy binary64 from the regions the library reports; a traversal started from the class
record a ray looks up returns the brute-force closest hit, the primitives that reach that t all lie under it (so the
hit primitive and the tie flag are the full record's), and rays the argument does not cover (a zero, infinite or NaN
direction component, an origin that is not finite or far outside the grid) take class 24.

Siblings of one leaf are disjoint subtrees that together with the leaf make up the tree
(test_bounce_entry_host.test_every_record_reaches_every_leaf_exactly_once), so the statements about leaves follow from
those about siblings, which is how they are checked here: a record's references are expanded by one level, a chain
node into the two siblings it pairs.
"""
from __future__ import annotations

import collections
import ctypes as C
import functools

import numpy as np
import pytest

from cudaraytracer_amd import abi, scenes
from cudaraytracer_amd._lib import lib
from test_bounce_entry_host import LEAF, NONE, ROOT_MARK, TABLE_SCENES, Tables, _prim_t, brute_force, tables, traverse

FORMS = (1, 2)
NCLS, FULL = abi.BOUNCE_CLASSES, abi.BOUNCE_CLASS_FULL
RAYS = 3000

ClassTables = collections.namedtuple("ClassTables", "T info records regions")

_fp = lambda a: a.ctypes.data_as(C.POINTER(C.c_float))
_up = lambda a: a.ctypes.data_as(C.POINTER(C.c_uint32))


def _desc(key):
    from test_bounce_entry_host import _SCENES
    return (_SCENES[key]() if key in _SCENES else key).desc()


@functools.lru_cache(maxsize=None)
def class_tables(key, form, node_limit=0) -> ClassTables:
    """The class tables of a scene, and its bounce-entry tables with the class nodes behind the chain nodes."""
    T = tables(key)
    d = _desc(key)
    L = lib()
    info = abi.BounceClassInfo()
    assert L.rt_bounce_class_entries_host(C.byref(d), form, node_limit, None, None, None, None, None, None, 0, None,
                                          C.byref(info)) == 0, L.rt_last_error()
    assert info.num_records == T.info.num_records
    assert info.first_class_node == T.info.num_nodes + T.info.num_chain_nodes
    rec = np.zeros((max(1, info.num_records) * NCLS, 4), np.uint32)
    n48 = np.zeros((max(1, info.num_class_nodes), 12), np.float32)
    refs = np.zeros(max(1, info.num_class_nodes), np.uint32)
    reg = np.zeros((max(1, info.num_records), 6), np.float64)
    if info.form:
        assert L.rt_bounce_class_entries_host(C.byref(d), form, node_limit, _up(rec), _fp(n48), _up(refs),
                                              reg.ctypes.data_as(C.POINTER(C.c_double)), None, None, 0, None,
                                              C.byref(info)) == 0
    records = np.stack([rec & 0xFFFF, rec >> 16], axis=2).reshape(-1, NCLS, 8).astype(np.int64)
    ext = T._replace(nodes48=np.concatenate([T.nodes48, n48[: info.num_class_nodes]]),
                     refs=np.concatenate([T.refs, refs[: info.num_class_nodes]]))
    for a in (records, reg, ext.nodes48, ext.refs):
        a.setflags(write=False)
    return ClassTables(ext, info, records[: info.num_records], reg[: info.num_records])


def classes_of(key, o, d):
    """The classes of rays as the kernel computes them (o = None: from the directions alone)."""
    dd = _desc(key)
    d32 = np.ascontiguousarray(d, np.float32)
    o32 = None if o is None else np.ascontiguousarray(o, np.float32)
    out = np.zeros(len(d32), np.uint32)
    info = abi.BounceClassInfo()
    assert lib().rt_bounce_class_entries_host(C.byref(dd), 0, 0, None, None, None, None, None if o is None else _fp(o32),
                                              _fp(d32), len(d32), _up(out), C.byref(info)) == 0, lib().rt_last_error()
    return out.astype(np.int64)


def cells_of(T: Tables, o):
    o32 = np.ascontiguousarray(o, np.float32)
    cells = np.zeros(len(o32), np.uint32)
    assert lib().rt_bounce_entry_cells(C.byref(T.info), _fp(o32), len(o32), _up(cells)) == 0
    return cells


def _siblings(T: Tables, e):
    """The sibling references (16-bit) behind the own leaf of record e, chain and class nodes expanded one level."""
    out = []
    for r in e[1:]:
        r = int(r)
        if r == NONE:
            continue
        if r < LEAF and r >= T.info.num_nodes:
            assert r < len(T.refs), f"reference {r} names no node"
            out += [int(T.refs[r]) & 0xFFFF, int(T.refs[r]) >> 16]
        else:
            out.append(r)
    return out


@functools.lru_cache(maxsize=None)
def _sibling_boxes(key):
    """16-bit child reference -> the box (lo.xyz, hi.xyz) its parent's 64-byte record holds for it."""
    T = tables(key)
    box = {}
    for n in range(T.info.num_nodes):
        r = T.nodes[n]
        c = r[12:14].view(np.int32)
        box[int(c[0]) & 0xFFFF] = np.array([r[0], r[2], r[8], r[1], r[3], r[9]], np.float64)
        box[int(c[1]) & 0xFFFF] = np.array([r[4], r[6], r[10], r[5], r[7], r[11]], np.float64)
    return box


def reachable(R, S, cls: int) -> bool:
    """rt_bounce_entry.h's box test: region R and sibling box S as (lo.xyz, hi.xyz) binary64, + - * and comparisons."""
    k = cls >> 3
    D = A = 0.0
    for j in range(3):
        D += max(R[3 + j], S[3 + j]) - min(R[j], S[j])
        A += max(abs(R[j]), abs(R[3 + j]), abs(S[j]), abs(S[3 + j]))
    m = 2.0 ** -8 * D + 2.0 ** -18 * A
    if not np.isfinite(m):
        return True
    neg_k = (cls >> k) & 1
    s = R[3 + k] - S[k] if neg_k else S[3 + k] - R[k]
    if s < -m:
        return False
    for j in range(3):
        if j == k:
            continue
        neg = (cls >> j) & 1
        lo, hi = (R[j] - s - m, R[3 + j]) if neg else (R[j], R[3 + j] + s + m)
        if S[3 + j] < lo - m or S[j] > hi + m:
            return False
    return True


# ----- (a) ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("key", TABLE_SCENES)
def test_class_24_is_the_full_record_and_form_0_builds_nothing(key):
    T = tables(key)
    for form in FORMS:
        CT = class_tables(key, form)
        assert CT.info.form in (1, 2) and CT.info.form <= form
        assert np.array_equal(CT.records[:, FULL, :], T.records)
        # the tables in front of the class nodes are rt_bounce_entries_host's
        assert np.array_equal(CT.T.nodes48[: len(T.nodes48)].view(np.uint32), T.nodes48.view(np.uint32))
        assert np.array_equal(CT.T.refs[: len(T.refs)], T.refs)
    assert class_tables(key, 1).info.num_class_nodes == 0
    off = class_tables(key, 0)
    assert off.info.form == 0 and off.info.num_class_nodes == 0 and off.info.num_records == T.info.num_records


# ----- (b), (c) -------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("key", TABLE_SCENES)
def test_class_records_hold_a_subset_and_leave_out_only_the_unreachable(key, form):
    CT = class_tables(key, form)
    T = CT.T
    box = _sibling_boxes(key)
    dropped = kept = 0
    for r in range(len(CT.records)):
        full = CT.records[r, FULL]
        R = CT.regions[r]
        if full[0] == ROOT_MARK or not R[0] <= R[3]:
            assert np.all(CT.records[r] == full[None, :]), "a root record, or one no cell names, keeps every class whole"
            continue
        assert np.all(np.isfinite(R)) and np.all(R[:3] < R[3:])
        whole = _siblings(T, full)
        assert len(set(whole)) == len(whole)
        for cls in range(FULL):
            e = CT.records[r, cls]
            assert e[0] == full[0] >= LEAF, "the own leaf is first"
            used = e[e != NONE]
            assert np.all(e[len(used):] == NONE), "the references are packed from the front"
            got = _siblings(T, e)
            assert len(set(got)) == len(got), "a sibling appears at most once"
            assert set(got) <= set(whole)
            # behind the leaf: at most one direct reference, then chain or class nodes
            assert all(T.info.num_nodes <= int(x) < LEAF for x in used[2:])
            for s in set(whole) - set(got):
                assert not reachable(R, box[s], cls), (r, cls, s)
                dropped += 1
            kept += len(got)
    print(f"{key} form {form}: {dropped} siblings dropped, {kept} kept over {len(CT.records)} records x 24 classes; "
          f"{CT.info.num_class_nodes} class nodes")
    if key in ("rtiow", "field"):
        assert dropped > 0


# ----- (f) ------------------------------------------------------------------------------------------------------

def _height(T: Tables, ref: int, memo) -> int:
    if ref >= LEAF:
        return 0
    if ref not in memo:
        memo[ref] = 1 + max(_height(T, c, memo) for c in (int(T.refs[ref]) & 0xFFFF, int(T.refs[ref]) >> 16))
    return memo[ref]


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("key", TABLE_SCENES)
def test_no_class_record_outgrows_the_stack(key, form):
    """test_bounce_entry_host.test_no_record_outgrows_the_stack's simulation on every (record, class)."""
    CT = class_tables(key, form)
    T, memo, depth = CT.T, {}, CT.T.info.depth
    for e in np.unique(CT.records.reshape(-1, 8), axis=0):
        if e[0] == ROOT_MARK:
            continue
        used = [int(r) for r in e[1:] if r != NONE]
        m = len(used)
        assert m <= 7 and m - 1 <= depth
        for j, r in enumerate(used):
            h = m - 1 - j
            if r >= LEAF:
                continue
            if r >= T.info.num_nodes:
                top = h + 1 + max(_height(T, c, memo) for c in (int(T.refs[r]) & 0xFFFF, int(T.refs[r]) >> 16))
            else:
                top = h + _height(T, r, memo)
            assert top <= depth, (e.tolist(), j, top, depth)


def test_scene_beyond_16_bit_references_has_no_class_table():
    d = scenes.sphere_field(9000, 6).desc()
    for form in (0, 1, 2):
        info = abi.BounceClassInfo()
        assert lib().rt_bounce_class_entries_host(C.byref(d), form, 0, None, None, None, None, None, None, 0, None,
                                                  C.byref(info)) == 0
        assert (info.form, info.num_records, info.num_class_nodes) == (0, 0, 0)
    o = np.zeros(3, np.float32)
    cls = np.zeros(1, np.uint32)
    assert lib().rt_bounce_class_entries_host(C.byref(d), 1, 0, None, None, None, None, _fp(o), _fp(o + 1), 1, _up(cls),
                                              C.byref(info)) < 0
    assert b"no bounce-entry table" in lib().rt_last_error()


def test_form_2_falls_back_to_form_1_at_the_node_limit():
    T = tables("rtiow")
    two = class_tables("rtiow", 2)
    assert two.info.form == 2 and two.info.num_class_nodes > 0
    first = two.info.first_class_node
    # a limit the re-paired table just fits, and one it just exceeds
    fits = class_tables("rtiow", 2, first + two.info.num_class_nodes + 1)
    assert fits.info.form == 2 and np.array_equal(fits.records, two.records)
    back = class_tables("rtiow", 2, first + two.info.num_class_nodes)
    assert back.info.form == 1 and back.info.num_class_nodes == 0
    assert np.array_equal(back.records, class_tables("rtiow", 1).records)
    assert len(back.T.refs) == len(T.refs)


# ----- (d), (e), (g): rays --------------------------------------------------------------------------------------

def _unit(rng, k):
    v = rng.normal(size=(k, 3))
    return v / np.linalg.norm(v, axis=1)[:, None]


def _ball(rng, k):
    return _unit(rng, k) * rng.uniform(size=(k, 1)) ** (1.0 / 3.0)


def _on_prims(T: Tables, rng, which):
    """Points on primitives `which` and the outward normals there."""
    P = T.prims.astype(np.float64)
    tag = T.prims[:, 7].view(np.uint32) & 15
    p, n = np.zeros((len(which), 3)), np.zeros((len(which), 3))
    for r, k in enumerate(which):
        q = P[k]
        if tag[k] == abi.RT_SPHERE:
            n[r] = _unit(rng, 1)[0]
            p[r] = q[0:3] + abs(q[3]) * n[r]
        else:
            ik, ia, ib = {abi.RT_XYRECT: (2, 0, 1), abi.RT_XZRECT: (1, 0, 2), abi.RT_YZRECT: (0, 1, 2)}[int(tag[k])]
            p[r, ik], p[r, ia], p[r, ib] = q[0], rng.uniform(q[1], q[2]), rng.uniform(q[3], q[4])
            n[r, ik] = rng.choice((-1.0, 1.0))
    return p, n


Rays = collections.namedtuple("Rays", "o d lambertian want at_best full_t")


@functools.lru_cache(maxsize=None)
def rays(key) -> Rays:
    """3 000 rays of a scene with their brute-force answers: (t, the primitives whose own test gives that t) and the
    traversal from the full record.  Computed once per scene."""
    T = tables(key)
    rng = np.random.default_rng(14)
    P = T.prims.astype(np.float64)
    tag = T.prims[:, 7].view(np.uint32) & 15
    org = np.array(list(T.info.grid_origin), np.float64)
    inv = np.array(list(T.info.grid_inv), np.float64)
    dim = np.array(list(T.info.grid_dim), np.float64)
    cell = np.where(inv > 0, 1.0 / np.where(inv > 0, inv, 1.0), 0.0)
    ext = dim * cell
    size = np.where(tag == abi.RT_SPHERE, np.abs(P[:, 3]), np.maximum(P[:, 2] - P[:, 1], P[:, 4] - P[:, 3]))
    g = int(np.argmax(size))

    def ground(points):  # the largest primitive's surface towards `points`, and its normal there
        if tag[g] == abi.RT_SPHERE:
            q = points - P[g, 0:3]
            n = q / np.linalg.norm(q, axis=1)[:, None]
            return P[g, 0:3] + abs(P[g, 3]) * n, n
        return _on_prims(T, rng, np.full(len(points), g))

    o, d = [], []
    # on primitive surfaces, Lambertian bounces n + q
    p, n = _on_prims(T, rng, rng.integers(0, len(P), 1000))
    o.append(p), d.append(n + _ball(rng, len(p)))
    # the ground inside the grid
    p, n = ground(org + rng.uniform(size=(800, 3)) * ext)
    o.append(p), d.append(n + _ball(rng, len(p)))
    # ... and outside it: up to one cell (still classified), and far (class 24)
    side = rng.choice((-1.0, 1.0), size=(300, 3))
    reach = np.where(rng.uniform(size=(300, 1)) < 0.5, rng.uniform(0.0, 1.5, size=(300, 3)) * cell,
                     rng.uniform(2.0, 30.0, size=(300, 3)) * (ext + 1.0))
    p, n = ground(org + 0.5 * ext + side * (0.5 * ext + reach * (rng.uniform(size=(300, 3)) < 0.6)))
    o.append(p), d.append(n + _ball(rng, len(p)))
    n_lambert = 2100
    # cell faces, edges and corners (lattice coordinates from one cell outside the grid to one beyond its far side)
    lattice = org + rng.integers(-1, dim.astype(np.int64) + 2, size=(500, 3)) * cell
    free = org - cell + rng.uniform(size=(500, 3)) * (ext + 2 * cell)
    o.append(np.where(rng.uniform(size=(500, 3)) < 0.6, lattice, free)), d.append(_unit(rng, 500))
    # special directions from surface points: axis-parallel, |d_x| = |d_y| (and the other pairs), tiny components
    p, n = _on_prims(T, rng, rng.integers(0, len(P), 400))
    s = _unit(rng, 400)
    kind = np.arange(400) % 4
    ax = rng.integers(0, 3, 400)
    for r in range(400):
        a, b = ax[r], (ax[r] + 1) % 3
        if kind[r] == 0:
            s[r] = 0.0
            s[r, a] = rng.choice((-1.0, 1.0))
        elif kind[r] == 1:
            s[r, b] = s[r, a] * rng.choice((-1.0, 1.0))
        elif kind[r] == 2:
            s[r, b] = rng.choice((-1.0, 1.0)) * rng.choice((1e-30, 1e-38, 1.5e-45, 1e-10))
        else:
            s[r, a] = s[r, b] = rng.choice((1e-20, -1e-20))
    o.append(p), d.append(s)
    o = np.concatenate(o).astype(np.float32).astype(np.float64)
    d = np.concatenate(d).astype(np.float32).astype(np.float64)
    assert len(o) == RAYS
    want = brute_force(T, o, d)
    # the primitives whose own test, on its own, gives the closest t: the hit primitive and whatever ties with it
    at_best = [[] for _ in range(RAYS)]
    hit = np.isfinite(want)
    inf = np.full(RAYS, np.inf)
    for k in range(len(P)):
        t = _prim_t(np.broadcast_to(P[k], (RAYS, 8)), o, d, inf)
        for r in np.nonzero(hit & (t == want))[0]:
            at_best[r].append(k)
    cells = cells_of(T, o)
    rec = T.records[T.grid[cells]]
    full_t, _ = traverse(T, o, d, [[0] if e[0] == ROOT_MARK else [int(x) for x in e if x != NONE] for e in rec])
    lam = np.zeros(RAYS, bool)
    lam[:n_lambert] = True
    for a in (o, d, want, full_t, lam):
        a.setflags(write=False)
    return Rays(o, d, lam, want, at_best, full_t)


def _leaves_under(T: Tables, ref: int, memo):
    if ref not in memo:
        if ref >= LEAF:
            memo[ref] = frozenset([ref])
        else:
            memo[ref] = _leaves_under(T, int(T.refs[ref]) & 0xFFFF, memo) | _leaves_under(T, int(T.refs[ref]) >> 16, memo)
    return memo[ref]


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("key", TABLE_SCENES)
def test_traversal_from_the_class_record_finds_the_closest_hit(key, form):
    CT = class_tables(key, form)
    T = CT.T
    Y = rays(key)
    cls = classes_of(key, Y.o, Y.d)
    rec = CT.records[T.grid[cells_of(T, Y.o)], cls]
    start = [[0] if e[0] == ROOT_MARK else [int(x) for x in e if x != NONE] for e in rec]
    got, visits = traverse(T, Y.o, Y.d, start)
    # (a NaN t: a rectangle's plane holds an axis-parallel ray; the same rays either way, and class 24's)
    assert np.array_equal(Y.full_t, Y.want, equal_nan=True)
    assert np.all(cls[np.isnan(Y.want)] == FULL)
    bad = np.nonzero((got != Y.want) & ~(np.isnan(got) & np.isnan(Y.want)))[0]
    assert len(bad) == 0, (len(bad), bad[:5].tolist(), got[bad[:5]].tolist(), Y.want[bad[:5]].tolist(), cls[bad[:5]].tolist())
    # the hit primitive and every primitive that ties with it lie under the record: same primitive, same tie flag
    memo = {}
    leaf_of = {}
    for l in _leaves_under(T, 0, memo):
        x = l ^ 0xFFFF
        for p in range(x >> 2, (x >> 2) + (x & 3) + 1):
            leaf_of[p] = l
    for r in np.nonzero(np.isfinite(Y.want))[0]:
        assert Y.at_best[r], r
        if start[r] == [0]:
            continue
        under = frozenset().union(*[_leaves_under(T, x, memo) for x in start[r]])
        assert all(leaf_of[p] in under for p in Y.at_best[r]), (r, Y.at_best[r], start[r])
    classified = (cls != FULL).sum()
    print(f"{key} form {form}: {classified} of {RAYS} rays classified, {np.isfinite(Y.want).sum()} hit; references "
          f"behind the leaf {np.mean([len(s) - 1 for s in start]):.2f}; node visits per ray {visits.mean():.2f}")
    assert classified > RAYS // 3


def test_rays_outside_the_argument_take_the_full_record():
    T = tables("rtiow")
    org = np.array(list(T.info.grid_origin), np.float64)
    inv = np.array(list(T.info.grid_inv), np.float64)
    dim = np.array(list(T.info.grid_dim), np.float64)
    cell = 1.0 / inv
    mid = org + 0.5 * dim * cell
    good_d = np.array([0.3, 1.0, -0.2])
    bad_d = [(0.0, 1.0, 0.2), (1.0, -0.0, 0.2), (1.0, 0.5, 0.0), (np.inf, 1.0, 1.0), (1.0, -np.inf, 1.0), (1.0, 1.0, np.nan),
             (np.nan, np.nan, np.nan), (0.0, 0.0, 0.0), (3e38, 3e38, 3e38)]
    cls = classes_of("rtiow", np.tile(mid, (len(bad_d), 1)), np.array(bad_d))
    assert np.all(cls == FULL), cls
    bad_o = [(np.nan, mid[1], mid[2]), (mid[0], np.inf, mid[2]), (mid[0], mid[1], -np.inf), (3e38, mid[1], mid[2])]
    for a in range(3):
        for s in (-1.0, 1.0):  # more than one cell below the grid, and beyond its far side
            p = mid.copy()
            p[a] = org[a] - 1.01 * cell[a] if s < 0 else org[a] + (dim[a] + 1.01) * cell[a]
            bad_o.append(tuple(p))
    cls = classes_of("rtiow", np.array(bad_o), np.tile(good_d, (len(bad_o), 1)))
    assert np.all(cls == FULL), cls
    # inside, on the grid's faces and up to (just under) one cell below it: classified, as the direction alone is
    ok_o = [mid, org, org + dim * cell * 0.999, org - 0.99 * cell * np.array([1.0, 0.0, 0.0]), org - 0.33 * cell]
    want = classes_of("rtiow", None, np.tile(good_d, (len(ok_o), 1)))
    assert np.all(want == 8 * 1 + 4) and np.array_equal(classes_of("rtiow", np.array(ok_o), np.tile(good_d, (len(ok_o), 1))), want)
    # the 24 classes: the dominant axis, then the three sign bits
    for k in range(3):
        for octant in range(8):
            v = np.array([0.3, 0.3, 0.3])
            v[k] = 1.0
            v = np.where((octant >> np.arange(3)) & 1, -v, v)
            assert classes_of("rtiow", None, v[None, :])[0] == 8 * k + octant


@pytest.mark.parametrize("form", FORMS)
def test_rtiow_class_records_are_shorter_on_lambertian_bounces(form):
    CT = class_tables("rtiow", form)
    Y = rays("rtiow")
    cls = classes_of("rtiow", Y.o, Y.d)
    idx = CT.T.grid[cells_of(CT.T, Y.o)]
    count = lambda e: (e[:, 1:] != NONE).sum(axis=1)[Y.lambertian].mean()
    full, got = count(CT.records[idx, FULL]), count(CT.records[idx, cls])
    print(f"rtiow form {form}: references behind the leaf per Lambertian bounce {full:.2f} -> {got:.2f}")
    assert got < full


# ----- arguments and layouts ------------------------------------------------------------------------------------

def test_arguments_and_struct_sizes():
    L = lib()
    assert C.sizeof(abi.BounceClassInfo) == 16 and C.sizeof(abi.BounceEntriesInfo) == 64
    assert (NCLS, FULL) == (25, 24)
    d = _desc("two")
    info = abi.BounceClassInfo()
    args = (None, None, None, None, None, None, 0, None)
    assert L.rt_bounce_class_entries_host(C.byref(d), 1, 0, *args, None) < 0 and b"info is NULL" in L.rt_last_error()
    for bad in (-2, 3):
        assert L.rt_bounce_class_entries_host(C.byref(d), bad, 0, *args, C.byref(info)) < 0
        assert b"form" in L.rt_last_error()
    assert L.rt_bounce_class_entries_host(C.byref(d), 1, 0x8000, *args, C.byref(info)) < 0 and b"node_limit" in L.rt_last_error()
    v = np.ones(3, np.float32)
    out = np.zeros(1, np.uint32)
    assert L.rt_bounce_class_entries_host(C.byref(d), 1, 0, None, None, None, None, None, None, 1, _up(out), C.byref(info)) < 0
    assert L.rt_bounce_class_entries_host(C.byref(d), 1, 0, None, None, None, None, None, _fp(v), 1, None, C.byref(info)) < 0
    assert L.rt_bounce_class_entries_host(None, 1, 0, *args, C.byref(info)) < 0
    # the switch: thread-local, returns the previous value, refuses other values; -1 reads it
    prev = L.rt_set_bounce_classes(2)
    assert prev in (0, 1, 2)
    try:
        assert L.rt_set_bounce_classes(1) == 2
        for bad in (-1, 3, 1 << 20):
            assert L.rt_set_bounce_classes(bad) < 0 and b"rt_set_bounce_classes" in L.rt_last_error()
        assert L.rt_bounce_class_entries_host(C.byref(_desc("ends")), -1, 0, *args, C.byref(info)) == 0 and info.form == 1
        assert L.rt_set_bounce_classes(0) == 1
        assert L.rt_bounce_class_entries_host(C.byref(_desc("ends")), -1, 0, *args, C.byref(info)) == 0 and info.form == 0
        # an explicit form leaves the thread's value alone
        assert L.rt_bounce_class_entries_host(C.byref(_desc("ends")), 2, 0, *args, C.byref(info)) == 0 and info.form == 2
        assert L.rt_set_bounce_classes(0) == 0
    finally:
        assert L.rt_set_bounce_classes(prev) >= 0
