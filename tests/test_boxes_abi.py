"""Box overlap queries (bm_scene_overlap_boxes): the triangle/box function restated, the brute force, the rules
by hand, the ABI's layout and null handling, the C++ layer, the conservativeness of the traversal's node test
walked over the oracle's BVH4 without a GPU, and the designed box sets the GPU tests use (CPU).

The yardstick is brute_boxes: tri_box below (the header's function in numpy float32, one rounding per
operation, in the order written) evaluated for every triangle and every valid box, on the triangle as the
build's record holds it: v0, v0 + e1, v0 + e2 with e1 = v1 - v0, e2 = v2 - v0. No value in it comes from the
library.
"""
import ctypes as C
import os
import subprocess

import numpy as np

from raytracercuda_amd import _lib, scenes

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
SIGNATURE = _lib.SIGNATURES["bm_scene_overlap_boxes"]  # the query all of this is about: no binding, no tests
EMPTY_REF, LEAF_BIT, FIRST_MASK = 0xFFFFFFFF, 0x80000000, 0x07FFFFFF

SNIPPET = r"""
#include <cstddef>
#include <beam/Beam.h>
static_assert(sizeof(bm_box) == 32 && offsetof(bm_box, center) == 0 && offsetof(bm_box, pad0) == 12 &&
              offsetof(bm_box, half) == 16 && offsetof(bm_box, pad1) == 28, "bm_box layout");
static_assert(BM_BOXES_COUNT == 0u && BM_BOXES_ANY == 1u && BM_BOXES_LIST == 2u, "constants");
int main() {
    auto scene = Beam::IScene::create();  // no device here: null
    if (!scene) return 0;
    uint32_t* ids = nullptr;
    return (int)(scene->overlapBoxes(nullptr, 0, BM_BOXES_COUNT, nullptr) +
                 scene->overlapBoxes(nullptr, 0, BM_BOXES_LIST, nullptr, ids, ids));
}
"""


# ---- the triangle/box function (include/beam_c.h, "box overlap queries") --------------------------------
def _sep(pa, pb, rad):
    lt = pa < pb
    mn, mx = np.where(lt, pa, pb), np.where(lt, pb, pa)
    return (mn > rad) | (mx < -rad)


def tri_box_parts(c, h, v0, v1, v2):
    """(a cross-axis test separates, an AABB test separates, the plane test passes) for box centres c and
    half-sizes h against triangles v0, v1, v2: float32 arrays (..., 3) that broadcast."""
    c, h, v0, v1, v2 = (np.asarray(a, F) for a in (c, h, v0, v1, v2))
    assert all(a.dtype == F for a in (c, h, v0, v1, v2))
    x, y, z = 0, 1, 2
    with np.errstate(all="ignore"):
        w0, w1, w2 = v0 - c, v1 - c, v2 - c
        f0, f1, f2 = w1 - w0, w2 - w1, w0 - w2

        def ax_x(f, a, b):
            return _sep(f[..., z] * a[..., y] - f[..., y] * a[..., z], f[..., z] * b[..., y] - f[..., y] * b[..., z],
                        np.abs(f[..., z]) * h[..., y] + np.abs(f[..., y]) * h[..., z])

        def ax_y(f, a, b):
            return _sep(-f[..., z] * a[..., x] + f[..., x] * a[..., z], -f[..., z] * b[..., x] + f[..., x] * b[..., z],
                        np.abs(f[..., z]) * h[..., x] + np.abs(f[..., x]) * h[..., z])

        def ax_z0(f, a, b):
            return _sep(f[..., y] * a[..., x] - f[..., x] * a[..., y], f[..., y] * b[..., x] - f[..., x] * b[..., y],
                        np.abs(f[..., y]) * h[..., x] + np.abs(f[..., x]) * h[..., y])

        def ax_z(f, a, b):  # b's value first
            return ax_z0(f, b, a)

        cross = (ax_x(f0, w0, w2) | ax_y(f0, w0, w2) | ax_z(f0, w1, w2) |
                 ax_x(f1, w0, w2) | ax_y(f1, w0, w2) | ax_z0(f1, w0, w1) |
                 ax_x(f2, w0, w1) | ax_y(f2, w0, w1) | ax_z(f2, w1, w2))
        mn = np.where(w1 < w0, w1, w0)
        mx = np.where(w1 > w0, w1, w0)
        mn = np.where(w2 < mn, w2, mn)
        mx = np.where(w2 > mx, w2, mx)
        box = ((mn > h) | (mx < -h)).any(axis=-1)
        nrm = np.stack([f0[..., y] * f1[..., z] - f0[..., z] * f1[..., y],
                        f0[..., z] * f1[..., x] - f0[..., x] * f1[..., z],
                        f0[..., x] * f1[..., y] - f0[..., y] * f1[..., x]], axis=-1)
        pos = nrm > 0
        lo = np.where(pos, -h - w0, h - w0)
        hi = np.where(pos, h - w0, -h - w0)
        dlo = (nrm[..., x] * lo[..., x] + nrm[..., y] * lo[..., y]) + nrm[..., z] * lo[..., z]
        dhi = (nrm[..., x] * hi[..., x] + nrm[..., y] * hi[..., y]) + nrm[..., z] * hi[..., z]
        plane = ~(dlo > 0) & (dhi >= 0)
    assert nrm.dtype == F and dlo.dtype == F
    return cross, box, plane


def aabb_separates(c, h, v0, v1, v2):
    """tri_box_parts' AABB test alone (the same statements)."""
    with np.errstate(all="ignore"):
        w0, w1, w2 = v0 - c, v1 - c, v2 - c
        mn = np.where(w1 < w0, w1, w0)
        mx = np.where(w1 > w0, w1, w0)
        mn = np.where(w2 < mn, w2, mn)
        mx = np.where(w2 > mx, w2, mx)
        return ((mn > h) | (mx < -h)).any(axis=-1)


def tri_box(c, h, v0, v1, v2):
    cross, box, plane = tri_box_parts(c, h, v0, v1, v2)
    return ~cross & ~box & plane


def record_vertices(verts):
    """The triangle as the build's 48-byte record holds it: v0, v0 + e1, v0 + e2 from verts (ntri, 3, 3)."""
    verts = np.asarray(verts, F).reshape(-1, 3, 3)
    v0 = verts[:, 0]
    e1, e2 = verts[:, 1] - v0, verts[:, 2] - v0
    return v0, v0 + e1, v0 + e2


def valid_boxes(centers, halves):
    with np.errstate(all="ignore"):
        return np.isfinite(centers).all(axis=1) & np.isfinite(halves).all(axis=1) & (halves >= 0).all(axis=1)


def brute_boxes(centers, halves, verts, pairs=1 << 20):
    """What bm_scene_overlap_boxes must find for boxes (n,3)+(n,3) over the triangles verts (ntri,3,3) in
    global-id order: {"count": (n,) uint32, "any": (n,) bool, "ids": list of n ascending id arrays}. Every
    triangle is tested for every valid box, chunked over boxes."""
    centers, halves = np.asarray(centers, F).reshape(-1, 3), np.asarray(halves, F).reshape(-1, 3)
    n = centers.shape[0]
    v0, v1, v2 = record_vertices(verts)
    ntri = v0.shape[0]
    ids = [np.zeros(0, np.uint32) for _ in range(n)]
    idx = np.flatnonzero(valid_boxes(centers, halves))
    if ntri and idx.size:
        step = max(1, pairs // ntri)
        for at in range(0, idx.size, step):
            sel = idx[at:at + step]
            # the function is a conjunction without side effects: its AABB part first, for every pair, and
            # the whole of it on the pairs that part does not separate
            r, g = np.nonzero(~aabb_separates(centers[sel, None, :], halves[sel, None, :], v0[None], v1[None], v2[None]))
            keep = tri_box(centers[sel[r]], halves[sel[r]], v0[g], v1[g], v2[g])
            r, g = r[keep], g[keep]  # row-major: ids ascending within a box
            cuts = np.searchsorted(r, np.arange(sel.size + 1))
            for j, i in enumerate(sel):
                ids[i] = g[cuts[j]:cuts[j + 1]].astype(np.uint32)
    count = np.array([a.size for a in ids], np.uint32)
    return {"count": count, "any": count > 0, "ids": ids}


def tri_vertices(meshes):
    """(ntri, 3, 3) vertex positions by global triangle id (scene order, then face order)."""
    return np.concatenate([np.asarray(m["pos"], F).reshape(-1, 3)[np.asarray(m["idx"]).reshape(-1, 3)]
                           for m in meshes] + [np.zeros((0, 3, 3), F)])


# ---- box sets ------------------------------------------------------------------------------------------
def grid_boxes(lo, hi, dims):
    """IScene.voxelize's cells, by the statements of its docstring: centres (n,3) and halves (n,3), cell
    (i, j, k) at row (i * ny + j) * nz + k."""
    lo32, hi32 = F(lo), F(hi)
    cell = (hi32 - lo32) / F(dims)
    half = F(0.5) * cell
    axes = [lo32[a] + (np.arange(dims[a], dtype=F) + F(0.5)) * cell[a] for a in range(3)]
    ctr = np.stack(np.meshgrid(*axes, indexing="ij"), axis=-1).reshape(-1, 3)
    assert ctr.dtype == F and half.dtype == F
    return np.ascontiguousarray(ctr), np.ascontiguousarray(np.broadcast_to(half, ctr.shape))


def bounds(verts):
    p = np.asarray(verts, F).reshape(-1, 3)
    return p.min(axis=0), p.max(axis=0)


def centroid_boxes(verts, every=16):
    """Boxes at every 16th triangle's centroid with a quarter of its longest edge as half-size on all axes."""
    t = np.asarray(verts, F)[::every]
    ctr = (t[:, 0] + t[:, 1] + t[:, 2]) / F(3)
    edge = np.stack([np.linalg.norm((t[:, a] - t[:, b]).astype(np.float64), axis=1) for a, b in ((1, 0), (2, 1), (0, 2))])
    half = F(0.25) * edge.max(axis=0).astype(F)
    return np.ascontiguousarray(ctr, F), np.ascontiguousarray(np.repeat(half[:, None], 3, axis=1), F)


def translated(meshes, shift):
    return [dict(m, pos=np.asarray(m["pos"], F).reshape(-1, 3) + F(shift)) for m in meshes]


SHIFTS = [(65536, 0, 0), (1000, -2000, 500)]


def sliver_meshes(n=240, seed=31):
    """Long slivers spanning magnitudes, one end near 1e-3 and the other near 1e3. Even triangles start at the
    far end: e1 = v1 - v0 rounds at the scale of v0 (an ulp of 6e-5 against a v1 of 1e-3), so v0 + e1 differs
    from the mesh's v1 (asserted by the tests). Odd triangles start at the near end, where v0 + e1 rounds back
    onto v1."""
    rng = np.random.default_rng(seed)
    near = rng.uniform(-1e-3, 1e-3, (n, 3))
    d = rng.normal(size=(n, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    far = d * rng.uniform(300, 1000, (n, 1))
    even = (np.arange(n) % 2 == 0)[:, None]
    v0, v1 = np.where(even, far, near), np.where(even, near, far)
    v2 = v1 + rng.normal(size=(n, 3)) * np.where(even, rng.uniform(1e-4, 1e-3, (n, 1)), rng.uniform(0.01, 3.0, (n, 1)))
    v = F(np.stack([v0, v1, v2], axis=1)).reshape(-1, 3)
    return [{"pos": v, "nrm": np.tile(F([0, 0, 1]), (v.shape[0], 1)), "idx": np.arange(v.shape[0], dtype=np.uint32)}]


def sliver_boxes(verts):
    lo, hi = bounds(verts)
    gc, gh = grid_boxes(lo, hi, (6, 6, 6))
    cc, ch = centroid_boxes(verts, every=4)
    # about the origin, where every sliver has one end: from a point to a box that holds them all
    oh = F([[1e-3] * 3, [1e-2] * 3, [1.0] * 3, [0] * 3, [50.0] * 3, [1e-4, 1, 1e-4], [1e3] * 3, [2e3] * 3])
    return np.concatenate([gc, cc, np.zeros((8, 3), F)]), np.concatenate([gh, ch, oh])


# ---- the rules, by hand ------------------------------------------------------------------------------
UP = np.nextafter(F(1), F(2))
RULES = [  # (what, triangle, box centre, box half, accepted)
    ("a vertex exactly on a face", [[1, .25, .25], [2, .5, 0], [2, 0, .5]], [0, 0, 0], [1, 1, 1], True),
    ("one ulp outside", [[UP, .25, .25], [2, .5, 0], [2, 0, .5]], [0, 0, 0], [1, 1, 1], False),
    ("an edge cuts the box, no vertex inside", [[-3, .5, 0], [3, .5, .25], [0, 6, 0]], [0, 0, 0], [1, 1, 1], True),
    ("the box inside a large triangle's plane region", [[-10, -10, .25], [10, -10, .25], [0, 15, .25]],
     [0, 0, 0], [1, 1, 1], True),
    ("AABBs overlap, a cross axis separates", [[3, -.5, 0], [-.5, 3, 0], [3, 3, 0]], [0, 0, 0], [1, 1, 1], False),
    ("only the plane test rejects", [[3.5, 0, 0], [0, 3.5, 0], [0, 0, 3.5]], [0, 0, 0], [1, 1, 1], False),
    ("the same plane, touching the corner", [[3, 0, 0], [0, 3, 0], [0, 0, 3]], [0, 0, 0], [1, 1, 1], True),
    ("half = 0 on the triangle", [[0, 0, 0], [2, 0, 0], [0, 2, 0]], [.5, .5, 0], [0, 0, 0], True),
    ("half = 0 off the triangle", [[0, 0, 0], [2, 0, 0], [0, 2, 0]], [.5, .5, .125], [0, 0, 0], False),
    ("a point triangle inside", [[.5, .5, .5]] * 3, [0, 0, 0], [1, 1, 1], True),
    ("a point triangle outside", [[2, 2, 2]] * 3, [0, 0, 0], [1, 1, 1], False),
    ("a collinear triangle through the box", [[-2, 0, 0], [2, 0, 0], [0, 0, 0]], [0, 0, 0], [1, 1, 1], True),
    ("a collinear triangle beside the box", [[-2, 3, 0], [2, 3, 0], [0, 3, 0]], [0, 0, 0], [1, 1, 1], False),
]
INVALID = [([np.nan, 0, 0], [1, 1, 1]), ([0, np.inf, 0], [1, 1, 1]), ([0, 0, -np.inf], [1, 1, 1]),
           ([0, 0, 0], [np.nan, 1, 1]), ([0, 0, 0], [1, np.inf, 1]), ([0, 0, 0], [1, 1, -1]),
           ([0, 0, 0], [-0.5, 1, 1]), ([0, 0, 0], [1, -1e-30, 1])]


def rule_scene():
    """The rule triangles as one scene (ids in RULES order), and the rule boxes followed by the invalid ones."""
    verts = F([r[1] for r in RULES])
    ctr = F([r[2] for r in RULES] + [b[0] for b in INVALID])
    half = F([r[3] for r in RULES] + [b[1] for b in INVALID])
    return verts, ctr, half


def test_rules_by_hand():
    for what, tri, c, h, want in RULES:
        t = F(tri)
        assert bool(tri_box(F(c), F(h), t[0], t[1], t[2])) == want, what
    parts = {r[0]: tri_box_parts(F(r[2]), F(r[3]), *F(r[1])) for r in RULES}
    cross, box, plane = parts["AABBs overlap, a cross axis separates"]
    assert cross and not box and plane
    cross, box, plane = parts["only the plane test rejects"]
    assert not cross and not box and not plane
    cross, box, plane = parts["one ulp outside"]
    assert box  # the AABB test, on fl(x - c) against h
    verts, ctr, half = rule_scene()
    exp = brute_boxes(ctr, half, verts)
    for i, r in enumerate(RULES):
        assert (i in exp["ids"][i].tolist()) == r[4], r[0]
    n = len(RULES)
    assert (exp["count"][n:] == 0).all() and not exp["any"][n:].any() and all(a.size == 0 for a in exp["ids"][n:])
    # half = 0 is valid: the origin is a vertex of triangles 7 and 8 and lies on the collinear triangle 11
    assert brute_boxes(F([[0, 0, 0]]), F([[0, 0, 0]]), verts)["ids"][0].tolist() == [7, 8, 11]
    assert brute_boxes(ctr, half, np.zeros((0, 3, 3), F))["count"].tolist() == [0] * ctr.shape[0]


def test_against_float64_on_random_pairs():
    """The restatement against an independent exact-geometry answer: in float64 the 13-axis SAT over the
    triangle's and the box's exact data. Away from contact (a relative gap of 1e-4 of the scale on the deciding
    axis) the two must agree."""
    rng = np.random.default_rng(3)
    n = 20000
    tri = rng.uniform(-2, 2, (n, 1, 3)) + rng.uniform(-1.5, 1.5, (n, 3, 3))
    c, h = rng.uniform(-1, 1, (n, 3)), rng.uniform(0.05, 1.5, (n, 3))
    got = tri_box(F(c), F(h), F(tri[:, 0]), F(tri[:, 1]), F(tri[:, 2]))
    t = F(tri).astype(np.float64) - F(c).astype(np.float64)[:, None, :]
    hh = F(h).astype(np.float64)
    edges = np.stack([t[:, 1] - t[:, 0], t[:, 2] - t[:, 1], t[:, 0] - t[:, 2]], axis=1)
    unit = np.eye(3)
    axes = [np.broadcast_to(unit[k], (n, 3)) for k in range(3)]
    axes += [np.cross(edges[:, e], unit[k]) for e in range(3) for k in range(3)]
    axes.append(np.cross(edges[:, 0], edges[:, 1]))
    gap = np.full(n, -np.inf)
    for a in axes:
        norm = np.maximum(np.linalg.norm(a, axis=1), 1e-300)
        p = np.einsum("nvk,nk->nv", t, a) / norm[:, None]
        r = (np.abs(a) * hh).sum(axis=1) / norm
        gap = np.maximum(gap, np.maximum(p.min(axis=1) - r, -p.max(axis=1) - r))
    clear = np.abs(gap) > 1e-4
    assert clear.mean() > 0.99 and 0.2 < got.mean() < 0.8
    assert np.array_equal(got[clear], (gap < 0)[clear])


# ---- ABI ---------------------------------------------------------------------------------------------
def test_record_layout_and_constants():
    assert C.sizeof(_lib.Box) == 32
    assert (_lib.Box.center.offset, _lib.Box.pad0.offset, _lib.Box.half.offset, _lib.Box.pad1.offset) == (0, 12, 16, 28)
    assert (_lib.BOXES_COUNT, _lib.BOXES_ANY, _lib.BOXES_LIST) == (0, 1, 2)
    res, args = SIGNATURE
    assert res is C.c_int32 and len(args) == 8
    assert len(_lib.SIGNATURES["bm_scene_overlap_boxes_counters"][1]) == 9
    assert {"bm_scene_overlap_boxes", "bm_scene_overlap_boxes_counters"} <= set(_lib.declared_symbols())


def test_null_scene_without_a_device():
    lib = _lib.load()
    out = (C.c_uint64 * 4)()
    bad = _lib.ERROR_INVALID_PARAMETER
    for mode in (0, 1, 2, 3):
        assert lib.bm_scene_overlap_boxes(None, None, 0, mode, 0, None, None, None) == bad
        assert lib.bm_scene_overlap_boxes(None, None, 16, mode, 0, None, None, None) == bad
        assert lib.bm_scene_overlap_boxes_counters(None, None, 0, mode, 0, None, None, None, out) == bad
    assert lib.bm_scene_overlap_boxes_counters(None, None, 0, 0, 0, None, None, None, None) == bad


def test_cpp_layer_compiles_and_links(tmp_path):
    """IScene::overlapBoxes of include/beam/Beam.h compiles and links against the library."""
    src = tmp_path / "boxes.cpp"
    src.write_text(SNIPPET)
    exe = tmp_path / "boxes"
    subprocess.run(["g++", "-std=c++17", "-O1", "-I", os.path.join(REPO, "include"), str(src), "-o", str(exe),
                    _lib.LIB_PATH, f"-Wl,-rpath,{os.path.dirname(_lib.LIB_PATH)}"], check=True)
    assert exe.exists()


# ---- the traversal loses nothing: the node test walked over the oracle's BVH4 ---------------------------
def walk(rec, tris, c, h):
    """The query's traversal in numpy over exported BVH4 records (n, 32) and triangle records (ntri, 12): a
    child is kept when ref != EMPTY_REF and, per axis, fl(lo - c) <= h and fl(hi - c) >= -h. Returns the global
    ids tri_box accepts among the leaves reached (ascending) and the number of leaf triangles tested."""
    box = rec[:, :24].view(F).reshape(-1, 6, 4)
    ref = rec[:, 24:28]
    tf = tris.view(F)
    found, tested = [], 0
    front = np.zeros(1 if tris.shape[0] else 0, np.int64)
    while front.size:
        b, r = box[front], ref[front]  # (m, 6, 4), (m, 4)
        with np.errstate(all="ignore"):
            keep = r != EMPTY_REF
            for a in range(3):
                keep &= (b[:, a, :] - c[a] <= h[a]) & (b[:, 3 + a, :] - c[a] >= -h[a])
        kept = r[keep]
        leaves = kept[(kept & LEAF_BIT) != 0]
        front = kept[(kept & LEAF_BIT) == 0].astype(np.int64)
        for lf in leaves:
            first, cnt = int(lf & FIRST_MASK), int((lf >> 27) & 15) + 1
            t = tf[first:first + cnt]
            v0 = t[:, 0:3]
            acc = tri_box(c, h, v0, v0 + t[:, 4:7], v0 + t[:, 8:11])
            found += tris[first:first + cnt, 3][acc].tolist()
            tested += cnt
    return np.sort(np.asarray(found, np.uint32)), tested


def leaf_boxes_hold_their_triangles(rec, tris):
    box = rec[:, :24].view(F).reshape(-1, 6, 4)
    ref = rec[:, 24:28]
    tf = tris.view(F)
    seen = 0
    for node, slot in zip(*np.nonzero((ref != EMPTY_REF) & ((ref & LEAF_BIT) != 0))):
        lf = ref[node, slot]
        first, cnt = int(lf & FIRST_MASK), int((lf >> 27) & 15) + 1
        t = tf[first:first + cnt]
        v0 = t[:, 0:3]
        pts = np.concatenate([v0, v0 + t[:, 4:7], v0 + t[:, 8:11]])
        lo, hi = box[node, 0:3, slot], box[node, 3:6, slot]
        assert (pts >= lo).all() and (pts <= hi).all(), (node, slot)
        seen += cnt
    return seen


def lemma_scenes():
    suz = scenes.load_mesh("suzanne")
    out = [("suzanne", suz)] + [(f"suzanne + {s}", translated(suz, s)) for s in SHIFTS]
    return out + [("slivers", sliver_meshes())]


def test_the_node_test_reaches_every_accepted_triangle(oracle):
    for name, meshes in lemma_scenes():
        verts = tri_vertices(meshes)
        rec, tris, _, _ = oracle.bvh_build(meshes, 4, width=4).export()
        assert rec.shape[1] == 32 and tris.shape[0] == verts.shape[0]
        assert leaf_boxes_hold_their_triangles(rec, tris) == verts.shape[0], name
        # the record's vertices are brute_boxes' (same two subtractions and additions)
        v0, v1, v2 = record_vertices(verts)
        tf, gid = tris.view(F), tris[:, 3]
        assert np.array_equal(tf[:, 0:3], v0[gid]) and np.array_equal(tf[:, 0:3] + tf[:, 4:7], v1[gid])
        if name == "slivers":
            ctr, half = sliver_boxes(verts)
            assert (v1 != verts[:, 1]).any(axis=1)[::2].mean() > 0.9  # v0 + e1 != v1: what the padding must cover
        else:
            lo, hi = bounds(verts)
            ctr, half = grid_boxes(lo, hi, (8, 8, 8))
            ctr, half = ctr[::3], half[::3]  # every third cell: the walk is a Python loop
            cc, ch = centroid_boxes(verts, every=64)
            ctr, half = np.concatenate([ctr, cc]), np.concatenate([half, ch])
        exp = brute_boxes(ctr, half, verts)
        assert exp["any"].any() and not exp["any"].all(), name
        tested = 0
        for i in range(ctr.shape[0]):
            got, t = walk(rec, tris, ctr[i], half[i])
            tested += t
            assert np.array_equal(got, exp["ids"][i]), (name, i)
        assert tested < 0.25 * ctr.shape[0] * verts.shape[0], name  # and it does prune
        lo, hi = bounds(verts)
        whole, t = walk(rec, tris, (lo + hi) * F(0.5), (hi - lo) * F(0.5) + F(1))
        assert whole.size == verts.shape[0] == t, name


# ---- the designed box sets ---------------------------------------------------------------------------
def suzanne_sets():
    """(verts, {"grid": the 8^3 grid over Suzanne's bounding box, "centroid": boxes at every 16th triangle})."""
    verts = tri_vertices(scenes.load_mesh("suzanne"))
    lo, hi = bounds(verts)
    return verts, {"grid": grid_boxes(lo, hi, (8, 8, 8)), "centroid": centroid_boxes(verts)}


def test_designed_sets_have_what_the_gpu_tests_need():
    verts, sets = suzanne_sets()
    assert verts.shape[0] == 15488
    ctr, half = sets["grid"]
    assert ctr.shape == (512, 3)
    grid = brute_boxes(ctr, half, verts)
    cnt = grid["count"].astype(np.int64)
    print(f"grid: empty {np.mean(cnt == 0):.3f}, 1..64 {np.mean((cnt > 0) & (cnt <= 64)):.3f}, "
          f"> 64 {np.mean(cnt > 64):.3f}, largest {cnt.max()}, sum {cnt.sum()}")
    assert np.mean(cnt == 0) >= 0.40 and np.mean(cnt > 64) >= 0.08
    ctr, half = sets["centroid"]
    assert ctr.shape == (968, 3)
    cen = brute_boxes(ctr, half, verts)
    cnt = cen["count"].astype(np.int64)
    assert (cnt >= 1).all()
    own = np.arange(0, verts.shape[0], 16)
    assert all(own[i] in cen["ids"][i] for i in range(own.size))  # each box holds the triangle it was made from
    shares = {"1..4": (cnt <= 4), "5..16": (cnt > 4) & (cnt <= 16), "17..64": (cnt > 16) & (cnt <= 64), "> 64": cnt > 64}
    print("centroid boxes: " + ", ".join(f"{k} {m.mean():.3f}" for k, m in shares.items()) +
          f", largest {cnt.max()}, sum {cnt.sum()}")
    assert shares["1..4"].mean() >= 0.40 and shares["5..16"].mean() >= 0.40
