"""Plane section queries (bm_scene_section_planes): the ABI's layout and null handling, the C++ layer, the rule
restated (tests/plane_scenes.py) against float64 and by hand, the bit-equality of the cut points of neighbouring
triangles, loop closure on the closed meshes, the conservativeness of the traversal's node test walked over the
oracle's BVH4 without a GPU, and chainSegments (CPU)."""
import ctypes as C
import os
import subprocess

import numpy as np

import plane_scenes as ps
from plane_scenes import F, U, brute_planes, crossed, cut_segments, plane_side
from raytracercuda_amd import _lib, beam, scenes

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIGNATURE = _lib.SIGNATURES["bm_scene_section_planes"]  # the query all of this is about: no binding, no tests
EMPTY_REF, LEAF_BIT, FIRST_MASK = 0xFFFFFFFF, 0x80000000, 0x07FFFFFF

SNIPPET = r"""
#include <cstddef>
#include <beam/Beam.h>
static_assert(sizeof(bm_plane) == 32 && offsetof(bm_plane, point) == 0 && offsetof(bm_plane, pad0) == 12 &&
              offsetof(bm_plane, normal) == 16 && offsetof(bm_plane, pad1) == 28, "bm_plane layout");
static_assert(sizeof(bm_segment) == 32 && offsetof(bm_segment, a) == 0 && offsetof(bm_segment, tri_id) == 12 &&
              offsetof(bm_segment, b) == 16 && offsetof(bm_segment, plane) == 28, "bm_segment layout");
static_assert(BM_PLANES_COUNT == 0u && BM_PLANES_ANY == 1u && BM_PLANES_LIST == 2u, "constants");
int main() {
    auto scene = Beam::IScene::create();  // no device here: null
    if (!scene) return 0;
    uint32_t* ids = nullptr;
    bm_segment* segs = nullptr;
    return (int)(scene->sectionPlanes(nullptr, 0, BM_PLANES_COUNT, nullptr) +
                 scene->sectionPlanes(nullptr, 0, BM_PLANES_LIST, nullptr, ids, ids, segs));
}
"""


# ---- ABI ---------------------------------------------------------------------------------------------------
def test_record_layout_and_constants():
    assert C.sizeof(_lib.Plane) == 32 and C.sizeof(_lib.Segment) == 32
    assert (_lib.Plane.point.offset, _lib.Plane.pad0.offset, _lib.Plane.normal.offset, _lib.Plane.pad1.offset) == (0, 12, 16, 28)
    assert (_lib.Segment.a.offset, _lib.Segment.tri_id.offset, _lib.Segment.b.offset, _lib.Segment.plane.offset) == (0, 12, 16, 28)
    assert (_lib.PLANES_COUNT, _lib.PLANES_ANY, _lib.PLANES_LIST) == (0, 1, 2)
    res, args = SIGNATURE
    assert res is C.c_int32 and len(args) == 9
    assert len(_lib.SIGNATURES["bm_scene_section_planes_counters"][1]) == 10
    assert {"bm_scene_section_planes", "bm_scene_section_planes_counters"} <= set(_lib.declared_symbols())


def test_null_scene_without_a_device():
    lib = _lib.load()
    out = (C.c_uint64 * 4)()
    bad = _lib.ERROR_INVALID_PARAMETER
    for mode in (0, 1, 2, 3):
        assert lib.bm_scene_section_planes(None, None, 0, mode, 0, None, None, None, None) == bad
        assert lib.bm_scene_section_planes(None, None, 16, mode, 0, None, None, None, None) == bad
        assert lib.bm_scene_section_planes_counters(None, None, 0, mode, 0, None, None, None, None, out) == bad
    assert lib.bm_scene_section_planes_counters(None, None, 0, 0, 0, None, None, None, None, None) == bad


def test_cpp_layer_compiles_and_links(tmp_path):
    """IScene::sectionPlanes of include/beam/Beam.h compiles and links against the library."""
    src = tmp_path / "planes.cpp"
    src.write_text(SNIPPET)
    exe = tmp_path / "planes"
    subprocess.run(["g++", "-std=c++17", "-O1", "-I", os.path.join(REPO, "include"), str(src), "-o", str(exe),
                    _lib.LIB_PATH, f"-Wl,-rpath,{os.path.dirname(_lib.LIB_PATH)}"], check=True)
    assert exe.exists()


# ---- the restatement ---------------------------------------------------------------------------------------
def test_against_float64_on_random_pairs():
    """The restated rule and cut points against a float64 evaluation of the exact float32 data, on plane/triangle
    pairs away from contact (every |s| above 1e-4 of its scale): the sides agree, and each cut point lies on the
    plane and on its edge to float32 accuracy."""
    assert SIGNATURE
    rng = np.random.default_rng(7)
    n = 20000
    tri = F(rng.uniform(-2, 2, (n, 1, 3)) + rng.uniform(-1.5, 1.5, (n, 3, 3)))
    pt, nr = F(rng.uniform(-2, 2, (n, 3))), F(rng.normal(size=(n, 3)))
    s = plane_side(pt[:, None, :], nr[:, None, :], tri)
    d64 = tri.astype(np.float64) - pt.astype(np.float64)[:, None, :]
    s64 = np.einsum("nvk,nk->nv", d64, nr.astype(np.float64))
    scale = np.linalg.norm(nr.astype(np.float64), axis=1)[:, None] * np.linalg.norm(d64, axis=2)
    clear = (np.abs(s64) > 1e-4 * scale).all(axis=1)
    assert clear.mean() > 0.99
    got = crossed(s)
    want = (s64 < 0).any(axis=1) & (s64 >= 0).any(axis=1)
    assert 0.2 < got.mean() < 0.9 and np.array_equal(got[clear], want[clear])
    sel = np.flatnonzero(got & clear)
    for i in sel[:2000]:
        a, b = cut_segments(pt[i], nr[i], tri[i][None])
        for X in (a[0], b[0]):
            x64 = X.astype(np.float64)
            assert abs(np.dot(x64 - pt[i], nr[i].astype(np.float64))) < 2e-5 * scale[i].max()
            # on one of the triangle's edges: collinear with its ends and between them
            t3 = tri[i].astype(np.float64)
            dist = min(np.linalg.norm(np.cross(t3[(k + 1) % 3] - t3[k], x64 - t3[k])) /
                       np.linalg.norm(t3[(k + 1) % 3] - t3[k]) for k in range(3))
            assert dist < 1e-5
        # seen from the front, the above side lies to the left of a -> b
        nt = np.cross(tri[i][1].astype(np.float64) - tri[i][0], tri[i][2].astype(np.float64) - tri[i][0])
        left = np.cross(nt, (b[0] - a[0]).astype(np.float64))
        assert np.dot(left, nr[i].astype(np.float64)) > 0


def test_rules_by_hand():
    assert SIGNATURE
    pt, nr = ps.RULE_PLANE
    for what, tri, want in ps.RULES:
        assert bool(crossed(plane_side(pt, nr, F(tri)))) == want, what
    verts, pts, nrm = ps.rule_scene()
    exp = brute_planes(pts, nrm, verts)
    assert exp["ids"][0].tolist() == [i for i, r in enumerate(ps.RULES) if r[2]]
    # every kind of invalid plane: not looked up
    assert (exp["count"][1:] == 0).all() and not exp["any"][1:].any() and all(s.shape[0] == 0 for s in exp["segs"][1:])
    assert not ps.valid_planes(pts[1:], nrm[1:]).any() and ps.valid_planes(pts[:1], nrm[:1]).all()
    seg = {int(r[3]): r for r in exp["segs"][0]}
    # touching from below in one vertex: a == b == that vertex's bits
    v = F(ps.RULES[1][1])[0]
    assert np.array_equal(seg[1][0:3], v.view(U)) and np.array_equal(seg[1][4:7], v.view(U))
    # touching from below with an edge: the segment is that edge, from x1 to x0 (the above side to the left)
    e = F(ps.RULES[3][1])
    assert np.array_equal(seg[3][0:3], e[1].view(U)) and np.array_equal(seg[3][4:7], e[0].view(U))
    assert (exp["segs"][0][:, 7] == 0).all()
    # the same triangle on a plane of the opposite normal: the sides swap, and so does what touching means
    flip = brute_planes(pt[None], -nr[None], verts)
    assert flip["ids"][0].tolist() == [0, 2, 7, 8, 10]
    assert brute_planes(pts, nrm, np.zeros((0, 3, 3), F))["count"].tolist() == [0] * pts.shape[0]


def test_orientation_in_all_six_sign_patterns():
    """One triangle, the plane z = 0 with normal +z, every pattern with both sides present: a is the cut of the
    edge leaving the above side, b of the edge returning to it, and above lies to the left of a -> b."""
    assert SIGNATURE
    xy = np.array([[0, 0], [4, 0], [0, 4]], np.float64)
    edge_of = {0: (0, 1), 1: (1, 2), 2: (2, 0)}
    seen = set()
    for bits in range(1, 7):
        below = [(bits >> k) & 1 == 1 for k in range(3)]
        z = [-1.0 if bl else 3.0 for bl in below]
        tri = F(np.column_stack([xy, z]))
        a, b = cut_segments(F([0, 0, 0]), F([0, 0, 1]), tri[None])
        dn = next(k for k in range(3) if not below[edge_of[k][0]] and below[edge_of[k][1]])
        up = next(k for k in range(3) if below[edge_of[k][0]] and not below[edge_of[k][1]])

        def cut(k):  # exact here: the heights are -1 and 3, so t = 1/4 from the below end
            i, j = edge_of[k]
            lo, hi = (i, j) if below[i] else (j, i)
            return tri[lo].astype(np.float64) + 0.25 * (tri[hi].astype(np.float64) - tri[lo])
        assert np.array_equal(a[0], F(cut(dn))) and np.array_equal(b[0], F(cut(up))), bits
        d = (b[0] - a[0]).astype(np.float64)
        assert a[0][2] == 0 and b[0][2] == 0
        # the triangle's front faces +z (counter-clockwise in xy): left of d is (-d.y, d.x); the above vertices
        # lie on that side
        left = np.array([-d[1], d[0]])
        for k in range(3):
            side = np.dot(left, xy[k] - a[0][:2].astype(np.float64))
            assert (side < 0) if below[k] else (side > 0), (bits, k)
        seen.add((dn, up))
    assert len(seen) == 6


def test_neighbours_compute_the_same_cut_bits():
    """Two triangles on one edge, opposite orientation, and again with the edge's vertices duplicated under other
    indices: the cut of the shared edge is bit-equal, whichever way each triangle runs along it."""
    assert SIGNATURE
    rng = np.random.default_rng(21)
    checked = 0
    for _ in range(400):
        p, q, r1, r2 = F(rng.uniform(-3, 3, (4, 3)))
        pt, nr = F(rng.uniform(-1, 1, 3)), F(rng.normal(size=3))
        sp, sq = plane_side(pt, nr, p), plane_side(pt, nr, q)
        if (sp < 0) == (sq < 0):
            continue
        one, two = np.stack([p, q, r1]), np.stack([q, p.copy(), r2])  # p -> q in one, q -> p in the other
        for rot in range(3):  # and wherever the edge sits in the index triple
            t1, t2 = np.roll(one, rot, axis=0), np.roll(two, -rot, axis=0)
            a1, b1 = cut_segments(pt, nr, t1[None])
            a2, b2 = cut_segments(pt, nr, t2[None])
            # the edge p-q runs downwards in one triangle and upwards in the other
            mine, theirs = (a1, b2) if not sp < 0 else (b1, a2)
            assert np.array_equal(mine.view(U), theirs.view(U))
            checked += 1
    assert checked > 300


def closed_cases():
    return [("torus",) + ps.torus_case(), ("icosphere",) + ps.icosphere_case()]


def test_closed_meshes_close_every_loop():
    """On the torus and the icosphere, over every plane of the designed sets: the sorted bytes of the a equal the
    sorted bytes of the b."""
    assert SIGNATURE
    total = 0
    for name, m, verts, pts, nrm, groups in closed_cases():
        assert ps.closed_manifold(m[0]), name
        assert verts.shape[0] == (768 if name == "torus" else 320)
        exp = brute_planes(pts, nrm, verts)
        for i in range(pts.shape[0]):
            assert ps.loop_closure(exp["segs"][i]), (name, i)
        cnt = exp["count"]
        # (a plane through a corner region of the bounding box may pass the mesh by: most random ones cross it)
        assert (cnt[groups["miss"]] == 0).all() and (cnt[groups["random"]] > 0).mean() >= 0.75
        assert (cnt[groups["vertex"]] > 0).all()
        assert (cnt[groups["rows"]] > 0).all()
        total += int(cnt.sum())
        print(f"{name}: {pts.shape[0]} planes, {int(cnt.sum())} crossed triangles, every plane closes")
    m, verts = ps.torus_case()[:2]
    assert np.sum(np.asarray(m[0]["pos"])[:, 2] == 0) == 48  # two rows of 24 vertices at z = 0
    # the plane z = 0: every triangle below with a vertex or an edge on it, nothing from above
    z0 = brute_planes(F([[0, 0, 0]]), F([[0, 0, 1]]), verts)
    seg = z0["segs"][0]
    zero = (seg[:, 0:3] == seg[:, 4:7]).all(axis=1)
    assert seg.shape[0] == 96 and zero.sum() == 48 and (verts[seg[:, 3]][:, :, 2] <= 0).all()
    assert total > 3000


# ---- the traversal loses nothing: the node test walked over the oracle's BVH4 -------------------------------
def walk(rec, tris, verts, pt, nr):
    """The query's traversal in numpy over exported BVH4 records (n, 32) and triangle records (ntri, 12): a child
    is kept when ref != EMPTY_REF, s at its corner lowest along the normal is < 0 and s at its corner highest
    along it is >= 0. Returns the global ids crossed among the leaves reached (ascending), on the meshes' own
    vertices verts (ntri,3,3), and the number of leaf triangles tested."""
    box = rec[:, :24].view(F).reshape(-1, 6, 4)
    ref = rec[:, 24:28]
    found, tested = [], 0
    front = np.zeros(1 if tris.shape[0] else 0, np.int64)
    pos = nr >= 0
    while front.size:
        b, r = box[front], ref[front]  # (m, 6, 4), (m, 4)
        lo, hi = np.moveaxis(b[:, 0:3, :], 1, 2), np.moveaxis(b[:, 3:6, :], 1, 2)  # (m, 4, 3)
        upper, lower = np.where(pos, hi, lo), np.where(pos, lo, hi)
        with np.errstate(all="ignore"):
            keep = (r != EMPTY_REF) & (plane_side(pt, nr, lower) < 0) & (plane_side(pt, nr, upper) >= 0)
        kept = r[keep]
        leaves = kept[(kept & LEAF_BIT) != 0]
        front = kept[(kept & LEAF_BIT) == 0].astype(np.int64)
        for lf in leaves:
            first, cnt = int(lf & FIRST_MASK), int((lf >> 27) & 15) + 1
            gid = tris[first:first + cnt, 3]
            found += gid[crossed(plane_side(pt, nr, verts[gid]))].tolist()
            tested += cnt
    return np.sort(np.asarray(found, U)), tested


def leaf_boxes_hold_the_mesh_vertices(rec, tris, verts):
    box = rec[:, :24].view(F).reshape(-1, 6, 4)
    ref = rec[:, 24:28]
    seen = 0
    for node, slot in zip(*np.nonzero((ref != EMPTY_REF) & ((ref & LEAF_BIT) != 0))):
        lf = ref[node, slot]
        first, cnt = int(lf & FIRST_MASK), int((lf >> 27) & 15) + 1
        pts = verts[tris[first:first + cnt, 3]].reshape(-1, 3)
        lo, hi = box[node, 0:3, slot], box[node, 3:6, slot]
        assert (pts >= lo).all() and (pts <= hi).all(), (node, slot)
        seen += cnt
    return seen


def lemma_scenes():
    from test_boxes_abi import sliver_meshes
    suz = scenes.load_mesh("suzanne")
    return [("suzanne", suz), ("suzanne + (65536, 0, 0)", ps.translated(suz, (65536, 0, 0))), ("slivers", sliver_meshes())]


def test_the_node_test_reaches_every_crossed_triangle(oracle):
    assert SIGNATURE
    for name, meshes in lemma_scenes():
        verts = ps.tri_vertices(meshes)
        rec, tris, _, _ = oracle.bvh_build(meshes, 4, width=4).export()
        assert rec.shape[1] == 32 and tris.shape[0] == verts.shape[0]
        assert leaf_boxes_hold_the_mesh_vertices(rec, tris, verts) == verts.shape[0], name
        if name == "slivers":  # the record's v0 + e1 is not the mesh's v1 here: the query reads the mesh
            tf = tris.view(F)
            assert (tf[:, 0:3] + tf[:, 4:7] != verts[tris[:, 3], 1]).any(axis=1).mean() > 0.4
        pts, nrm, groups = ps.designed_planes(verts, seed=5)
        exp = brute_planes(pts, nrm, verts)
        assert exp["any"].any() and not exp["any"].all(), name
        tested = 0
        for i in range(pts.shape[0]):
            got, t = walk(rec, tris, verts, pts[i], nrm[i])
            tested += t
            assert np.array_equal(got, exp["ids"][i]), (name, i)
        print(f"{name}: {tested / (pts.shape[0] * verts.shape[0]):.3f} of all plane/triangle pairs tested")
        if name != "slivers":  # (every sliver has an end at the origin: their boxes nest, little can be pruned)
            assert tested < 0.5 * pts.shape[0] * verts.shape[0], name  # and it does prune


# ---- chainSegments -----------------------------------------------------------------------------------------
def section(verts, pt, nr):
    seg = brute_planes(F([pt]), F([nr]), verts)["segs"][0]
    return np.ascontiguousarray(seg[:, 0:3]).view(F), np.ascontiguousarray(seg[:, 4:7]).view(F)


def check_runs(a, b, loops, chains):
    used = [i for run in loops + chains for i in run]
    live = [i for i in range(a.shape[0]) if a[i].tobytes() != b[i].tobytes()]
    assert sorted(used) == live  # every segment of positive length once
    for run in loops + chains:
        for i, j in zip(run[:-1], run[1:]):
            assert b[i].tobytes() == a[j].tobytes()
    for run in loops:
        assert b[run[-1]].tobytes() == a[run[0]].tobytes() and run[0] == min(run)


def test_chain_segments():
    assert SIGNATURE
    torus = ps.tri_vertices(ps.torus())
    a, b = section(torus, (0, 0, 0), (0, 0, 1))  # the vertex rows at z = 0: the outer and the inner equator
    loops, chains = beam.chainSegments(a, b)
    check_runs(a, b, loops, chains)
    assert len(loops) == 2 and not chains and sorted(len(r) for r in loops) == [24, 24]
    a, b = section(torus, (0, 0, 0), (0, 1, 0))  # through the hole's axis: the two circular cross-sections
    loops, chains = beam.chainSegments(a, b)
    check_runs(a, b, loops, chains)
    assert len(loops) == 2 and not chains
    a, b = section(torus, (0, 0, 0.3), (0.1, -0.2, 1))  # a general plane through the hole: two loops again
    loops, chains = beam.chainSegments(a, b)
    check_runs(a, b, loops, chains)
    assert len(loops) == 2 and not chains
    ball = ps.tri_vertices(ps.icosphere())
    a, b = section(ball, (0.25, -0.5, 0.2), (0.3, 0.2, 1))
    loops, chains = beam.chainSegments(a, b)
    check_runs(a, b, loops, chains)
    assert len(loops) == 1 and not chains and len(loops[0]) > 10
    # one crossed triangle removed: the loop opens into one chain
    seg = brute_planes(F([[0.25, -0.5, 0.2]]), F([[0.3, 0.2, 1]]), ball)["segs"][0]
    live = seg[~(seg[:, 0:3] == seg[:, 4:7]).all(axis=1)]
    holed = np.delete(ball, int(live[3, 3]), axis=0)
    a, b = section(holed, (0.25, -0.5, 0.2), (0.3, 0.2, 1))
    loops, chains = beam.chainSegments(a, b)
    check_runs(a, b, loops, chains)
    assert not loops and len(chains) == 1 and len(chains[0]) == live.shape[0] - 1
    # several segments starting at one point pair in ascending input order; zero-length ones are dropped
    P, Q, R, S = F([0, 0, 0]), F([1, 0, 0]), F([0, 1, 0]), F([0, 0, 1])
    a = np.stack([Q, P, R, P, S, S])
    b = np.stack([P, Q, P, R, S, P])
    loops, chains = beam.chainSegments(a, b)  # ends at P: 0, 2, 5; starts at P: 1, 3
    assert loops == [[0, 1], [2, 3]] and chains == [[5]]
    assert beam.chainSegments(np.zeros((0, 3), F), np.zeros((0, 3), F)) == ([], [])
