"""Triangle overlap queries (bm_scene_overlap_triangles): the triangle/triangle function restated, the brute
force, the rules by hand, the ABI's layout and null handling, the C++ layer, the conservativeness of the
traversal's node test walked over the oracle's BVH4 without a GPU, and the designed query set the GPU tests use
(CPU).

The yardstick is brute_tris: tri_tri below (the header's function in numpy float32, one rounding per operation,
in the order written) evaluated for every scene triangle and every valid query triangle, on the scene triangle
as the build's record holds it: v0, v0 + e1, v0 + e2 with e1 = v1 - v0, e2 = v2 - v0. No value in it comes from
the library.
"""
import ctypes as C
import os
import subprocess

import numpy as np

from raytracercuda_amd import _lib, scenes
from test_boxes_abi import (EMPTY_REF, FIRST_MASK, LEAF_BIT, SHIFTS, leaf_boxes_hold_their_triangles, record_vertices,
                            sliver_meshes, translated, tri_vertices)

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
SIGNATURE = _lib.SIGNATURES["bm_scene_overlap_triangles"]  # the query all of this is about: no binding, no tests
NO_TRI = 0xFFFFFFFF

SNIPPET = r"""
#include <cstddef>
#include <beam/Beam.h>
static_assert(sizeof(bm_tri) == 48 && offsetof(bm_tri, v0) == 0 && offsetof(bm_tri, pad0) == 12 &&
              offsetof(bm_tri, v1) == 16 && offsetof(bm_tri, pad1) == 28 && offsetof(bm_tri, v2) == 32 &&
              offsetof(bm_tri, pad2) == 44, "bm_tri layout");
static_assert(BM_TRIS_COUNT == 0u && BM_TRIS_ANY == 1u && BM_TRIS_LIST == 2u && BM_TRIS_PAD_SKIP_TRI == 1u,
              "constants");
int main() {
    auto scene = Beam::IScene::create();  // no device here: null
    if (!scene) return 0;
    uint32_t* ids = nullptr;
    return (int)(scene->overlapTriangles(nullptr, 0, BM_TRIS_COUNT, nullptr) +
                 scene->overlapTriangles(nullptr, 0, BM_TRIS_LIST, nullptr, ids, ids, BM_TRIS_PAD_SKIP_TRI));
}
"""


# ---- the triangle/triangle function (include/beam_c.h, "triangle overlap queries") -------------------------
def _dot(u, v):
    return (u[..., 0] * v[..., 0] + u[..., 1] * v[..., 1]) + u[..., 2] * v[..., 2]


def _cross(u, v):
    return np.stack([u[..., 1] * v[..., 2] - u[..., 2] * v[..., 1],
                     u[..., 2] * v[..., 0] - u[..., 0] * v[..., 2],
                     u[..., 0] * v[..., 1] - u[..., 1] * v[..., 0]], axis=-1)


def _bounds3(a, b, c):
    lo = np.where(b < a, b, a)
    hi = np.where(b > a, b, a)
    return np.where(c < lo, c, lo), np.where(c > hi, c, hi)


def _sep(d, p1, p2, q0, q1, q2):
    s1, s2 = _dot(d, p1), _dot(d, p2)
    zero = np.zeros_like(s1)
    mna, mxa = _bounds3(zero, s1, s2)
    mnb, mxb = _bounds3(_dot(d, q0), _dot(d, q1), _dot(d, q2))
    return (mxa < mnb) | (mxb < mna)


AXES = ["nA", "nB"] + [f"eA{i} x eB{j}" for i in range(3) for j in range(3)] + \
       [f"nA x eA{i}" for i in range(3)] + [f"nB x eB{j}" for j in range(3)]
IN_PLANE = slice(11, 17)


def aabb_meets(a0, a1, a2, b0, b1, b2):
    """tri_tri's AABB part: per axis min_j b_j <= qhi and max_j b_j >= qlo, on the raw coordinates."""
    with np.errstate(all="ignore"):
        qlo, qhi = _bounds3(a0, a1, a2)
        blo, bhi = _bounds3(b0, b1, b2)
        return ((blo <= qhi) & (bhi >= qlo)).all(axis=-1)


def sat_axes(a0, a1, a2, b0, b1, b2):
    """tri_tri's separating-axis part in the arrays' own dtype: (..., 17) bool, True where the axis separates, and
    the axes (17, ..., 3) with the translated vertices (p1, p2, q0, q1, q2)."""
    with np.errstate(all="ignore"):
        p1, p2 = a1 - a0, a2 - a0
        q0, q1, q2 = b0 - a0, b1 - a0, b2 - a0
        ea = [p1, p2 - p1, np.zeros_like(p2) - p2]
        eb = [q1 - q0, q2 - q1, q0 - q2]
        na, nb = _cross(ea[0], ea[1]), _cross(eb[0], eb[1])
        axes = [na, nb] + [_cross(ea[i], eb[j]) for i in range(3) for j in range(3)]
        axes += [_cross(na, ea[i]) for i in range(3)] + [_cross(nb, eb[j]) for j in range(3)]
        sep = np.stack([_sep(d, p1, p2, q0, q1, q2) for d in axes], axis=-1)
    return sep, axes, (p1, p2, q0, q1, q2)


def tri_tri_parts(a0, a1, a2, b0, b1, b2):
    """(the AABB part meets, (..., 17) which axes separate) for query triangles a and scene triangles b: float32
    arrays (..., 3) that broadcast."""
    a0, a1, a2, b0, b1, b2 = np.broadcast_arrays(*(np.asarray(x, F) for x in (a0, a1, a2, b0, b1, b2)))
    sep, axes, _ = sat_axes(a0, a1, a2, b0, b1, b2)
    assert axes[5].dtype == F and sep.shape[-1] == 17
    return aabb_meets(a0, a1, a2, b0, b1, b2), sep


def tri_tri(a0, a1, a2, b0, b1, b2, in_plane=True):
    meets, sep = tri_tri_parts(a0, a1, a2, b0, b1, b2)
    if not in_plane:
        sep = sep[..., :11]
    return meets & ~sep.any(axis=-1)


def valid_tris(q):
    return np.isfinite(q.reshape(-1, 9)).all(axis=1)


def brute_tris(queries, verts, skip=None, pairs=1 << 21):
    """What bm_scene_overlap_triangles must find for query triangles (n,3,3) over the scene triangles verts
    (ntri,3,3) in global-id order: {"count": (n,) uint32, "any": (n,) bool, "ids": list of n ascending id arrays}.
    The AABB part is evaluated for every pair of a valid query, the seventeen axes for the pairs that part keeps
    (the function is a conjunction without side effects). skip: None, or n ids removed from the accepted sets."""
    queries = np.asarray(queries, F).reshape(-1, 3, 3)
    n = queries.shape[0]
    b0, b1, b2 = record_vertices(verts)
    ntri = b0.shape[0]
    ids = [np.zeros(0, np.uint32) for _ in range(n)]
    idx = np.flatnonzero(valid_tris(queries))
    if ntri and idx.size:
        step = max(1, pairs // ntri)
        for at in range(0, idx.size, step):
            sel = idx[at:at + step]
            a = queries[sel]
            r, g = np.nonzero(aabb_meets(a[:, None, 0], a[:, None, 1], a[:, None, 2], b0[None], b1[None], b2[None]))
            keep = tri_tri(a[r, 0], a[r, 1], a[r, 2], b0[g], b1[g], b2[g])
            if skip is not None:
                keep &= g != np.asarray(skip, np.int64)[sel[r]]
            r, g = r[keep], g[keep]  # row-major: ids ascending within a query
            cuts = np.searchsorted(r, np.arange(sel.size + 1))
            for j, i in enumerate(sel):
                ids[i] = g[cuts[j]:cuts[j + 1]].astype(np.uint32)
    count = np.array([a.size for a in ids], np.uint32)
    return {"count": count, "any": count > 0, "ids": ids}


# ---- query sets ------------------------------------------------------------------------------------------
ROT_AXIS, ROT_ANGLE, ROT_SHIFT = (0.0, 0.0, 1.0), 0.02, (0.0002, 0.0001, -0.0002)


def moved(verts, origin=(0, 0, 0)):
    """verts (..., 3) turned by ROT_ANGLE about ROT_AXIS through `origin` and shifted by ROT_SHIFT: float64
    arithmetic, rounded once to float32. The fixed placement of the second mesh of the designed query sets."""
    k = np.asarray(ROT_AXIS, np.float64)
    k /= np.linalg.norm(k)
    kx = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    rot = np.eye(3) + np.sin(ROT_ANGLE) * kx + (1 - np.cos(ROT_ANGLE)) * (kx @ kx)
    o = np.asarray(origin, np.float64)
    return F((np.asarray(verts, np.float64) - o) @ rot.T + o + np.asarray(ROT_SHIFT, np.float64))


def suzanne_queries(shift=(0, 0, 0), every=16):
    """(scene verts, queries): Suzanne moved by `shift`, and every 16th triangle of a second Suzanne placed by
    moved() about the first one's position, so that the two interpenetrate."""
    verts = tri_vertices(translated(scenes.load_mesh("suzanne"), shift))
    return verts, np.ascontiguousarray(moved(verts[::every], origin=F(shift)))


def sliver_queries(verts):
    """Queries for the sliver scene: every 4th sliver turned and shifted about the origin, and triangles about
    the origin, where every sliver has one end, from tiny to one that spans them all."""
    rng = np.random.default_rng(41)
    near = [F(rng.normal(size=(3, 3)) * s) for s in (1e-4, 1e-3, 1e-2, 1.0, 50.0, 1e3, 3e3)]
    return np.concatenate([moved(verts[::4]), np.stack(near), verts[1::16]])


# ---- the rules, by hand ------------------------------------------------------------------------------------
UNIT = [[0, 0, 0], [1, 0, 0], [0, 1, 0]]
UP = float(np.nextafter(F(1), F(2)))
RULES = [  # (what, query triangle a, scene triangle b, accepted)
    ("a shared vertex", UNIT, [[0, 0, 0], [-1, 0, 1], [0, -1, 1]], True),
    ("a shared edge", UNIT, [[0, 0, 0], [1, 0, 0], [0, -1, 1]], True),
    ("two edges crossing in space", [[0, 0, 0], [2, 0, 0], [1, 0, -1]], [[1, -1, 0], [1, 1, 0], [1, 0, 1]], True),
    ("a vertex on the other's interior", [[.25, .25, 0], [.25, .25, 1], [1, 1, 1]], UNIT, True),
    ("an edge through the other's interior", [[.25, .25, -.5], [.25, .25, 1], [1, 1, 1]], UNIT, True),
    ("identical triangles", UNIT, UNIT, True),
    ("coplanar, overlapping", [[0, 0, 0], [2, 0, 0], [0, 2, 0]], [[.5, .5, 0], [3, .5, 0], [.5, 3, 0]], True),
    ("coplanar, one inside the other", [[0, 0, 0], [2, 0, 0], [0, 2, 0]], [[.25, .25, 0], [.75, .25, 0], [.25, .75, 0]],
     True),
    ("coplanar, apart", UNIT, [[.75, .75, 0], [2, .75, 0], [.75, 2, 0]], False),
    ("parallel planes one ulp apart", [[0, 0, 1], [1, 0, 1], [0, 1, 1]], [[0, 0, UP], [1, 0, UP], [0, 1, UP]], False),
    ("tilted parallel planes one ulp apart", [[0, 0, 0], [1, 0, 1], [0, 1, 1]],
     [[0, 0, UP - 1], [1, 0, UP], [0, 1, UP]], False),
    ("AABBs overlap, only a cross axis separates", [[0, 0, 0], [4, 0, 0], [2, 1, 4]], [[2, 3, 1], [2, -1, -1], [6, 2, -2]],
     False),
    ("only nA separates", [[2, -1.5, -1.5], [-.5, .5, .5], [1.5, -.5, 2]], [[-2, -.5, 2], [1, -.5, 1.5], [0, -1, .5]], False),
    ("only nB separates", [[-2, -.5, 1.5], [-.5, 0, 0], [-1.5, 0, -.5]], [[1, -1, .5], [-1, 2, 1.5], [0, -.5, -2]], False),
    ("a point-like query on the triangle", [[.25, .25, 0]] * 3, UNIT, True),
    ("a point-like query above the triangle", [[.25, .25, .125]] * 3, UNIT, False),
    ("a point-like query in the plane, beside", [[.75, .75, 0]] * 3, UNIT, False),
    ("a segment-like query through the triangle", [[.25, .25, -1], [.25, .25, 1], [.25, .25, 0]], UNIT, True),
    ("a segment-like query beside the triangle", [[.75, .75, -1], [.75, .75, 1], [.75, .75, 0]], UNIT, False),
    ("a point-like scene triangle on the query", UNIT, [[.25, .25, 0]] * 3, True),
    ("a point-like scene triangle off the query", UNIT, [[.25, .25, .125]] * 3, False),
    ("a segment-like scene triangle through the query", UNIT, [[.25, .25, -1], [.25, .25, 1], [.25, .25, 0]], True),
    ("a segment-like scene triangle beside the query", UNIT, [[.75, .75, -1], [.75, .75, 1], [.75, .75, 0]], False),
    ("two point-like triangles at one place", [[.5, .5, .5]] * 3, [[.5, .5, .5]] * 3, True),
]
INVALID = []
for _v in range(3):
    for _k in range(3):
        _t = np.array(UNIT, np.float64)
        _t[_v, _k] = (np.nan, np.inf, -np.inf)[(_v + _k) % 3]
        INVALID.append(_t.tolist())
INVALID.append([[np.nan] * 3] * 3)


def rule_scene():
    """The rules' scene triangles as one scene (ids in RULES order), and the rules' query triangles followed by
    the invalid ones."""
    verts = F([r[2] for r in RULES])
    queries = F([r[1] for r in RULES] + INVALID)
    return verts, queries


def test_rules_by_hand():
    parts = {}
    for what, a, b, want in RULES:
        a, b = F(a), F(b)
        assert bool(tri_tri(a[0], a[1], a[2], b[0], b[1], b[2])) == want, what
        parts[what] = tri_tri_parts(a[0], a[1], a[2], b[0], b[1], b[2])
    meets, sep = parts["coplanar, apart"]
    assert meets and not sep[:11].any() and sep[IN_PLANE].any()  # the six in-plane axes are what rejects it
    a, b = F(UNIT), F(RULES[8][2])
    assert RULES[8][0] == "coplanar, apart" and tri_tri(a[0], a[1], a[2], b[0], b[1], b[2], in_plane=False)
    meets, sep = parts["parallel planes one ulp apart"]
    assert not meets and sep[0] and sep[1]
    meets, sep = parts["tilted parallel planes one ulp apart"]
    assert meets and sep[0] and sep[1]  # the AABBs overlap: only the normals tell
    meets, sep = parts["AABBs overlap, only a cross axis separates"]
    assert meets and sep[2:11].any() and not sep[:2].any() and not sep[IN_PLANE].any()
    meets, sep = parts["only nA separates"]
    assert meets and np.flatnonzero(sep).tolist() == [0]
    meets, sep = parts["only nB separates"]
    assert meets and np.flatnonzero(sep).tolist() == [1]
    meets, sep = parts["a point-like query in the plane, beside"]
    assert meets and not sep[:14].any() and sep[14:].any()  # nB x eB: all a point has left in the plane
    meets, sep = parts["a segment-like query beside the triangle"]
    assert meets and not sep[:2].any()
    verts, queries = rule_scene()
    exp = brute_tris(queries, verts)
    for i, r in enumerate(RULES):
        assert (i in exp["ids"][i].tolist()) == r[3], r[0]
    n = len(RULES)
    assert len(INVALID) == 10 and not valid_tris(queries[n:]).any() and valid_tris(queries[:n]).all()
    assert (exp["count"][n:] == 0).all() and not exp["any"][n:].any() and all(a.size == 0 for a in exp["ids"][n:])
    assert brute_tris(queries, np.zeros((0, 3, 3), F))["count"].tolist() == [0] * queries.shape[0]
    # the skip filter takes the named id out of an accepted set and nothing else
    skip = np.arange(queries.shape[0])
    cut = brute_tris(queries, verts, skip=skip)
    for i in range(n):
        assert cut["ids"][i].tolist() == [g for g in exp["ids"][i].tolist() if g != i]


def test_against_float64_on_random_pairs():
    """The float32 restatement against the same seventeen-axis test in float64 on the same float32 inputs, on
    20,000 random pairs away from contact. "Away": the float64 test's deciding gap — over the axes that do not
    vanish, the largest of (minB - maxA, minA - maxB) divided by the axis' length: negative when the triangles
    intersect, the distance along the best axis when they do not — is larger in magnitude than 1e-3 of the pair's
    extent (its largest translated coordinate, about 5 here).
    Why 1e-3: a float32 projection carries about 10 roundings of 2^-24 relative to |d| * extent, and an axis
    d = u x v computed in float32 is turned from the exact one by about 2^-24 / sin(u, v); for the axes that can
    decide a random pair sin(u, v) is above 1e-2 but for a handful of the 20,000 * 15 crosses, so the float32 gap
    is off by at most 10 * 6e-8 * 1e2 = 6e-5 of the extent. 1e-3 leaves a factor of 16 and still keeps more than
    97 % of the pairs (asserted)."""
    rng = np.random.default_rng(5)
    n = 20000
    a = F(rng.uniform(-2, 2, (n, 1, 3)) + rng.uniform(-1.5, 1.5, (n, 3, 3)))
    b = F(a[:, :1].astype(np.float64) + rng.uniform(-0.3, 0.3, (n, 1, 3)) + rng.uniform(-1.5, 1.5, (n, 3, 3)))
    got = tri_tri(a[:, 0], a[:, 1], a[:, 2], b[:, 0], b[:, 1], b[:, 2])
    a64, b64 = a.astype(np.float64), b.astype(np.float64)
    sep, axes, (p1, p2, q0, q1, q2) = sat_axes(a64[:, 0], a64[:, 1], a64[:, 2], b64[:, 0], b64[:, 1], b64[:, 2])
    assert axes[0].dtype == np.float64
    want = ~sep.any(axis=-1)
    extent = np.max(np.abs(np.stack([p1, p2, q0, q1, q2])), axis=(0, 2))
    gap = np.full(n, -np.inf)
    for d in axes:
        norm = np.linalg.norm(d, axis=1)
        ok = norm > 1e-12
        u = d / np.where(ok, norm, 1.0)[:, None]
        pa = np.stack([np.zeros(n), _dot(u, p1), _dot(u, p2)])
        pb = np.stack([_dot(u, q0), _dot(u, q1), _dot(u, q2)])
        g = np.maximum(pb.min(axis=0) - pa.max(axis=0), pa.min(axis=0) - pb.max(axis=0))
        gap = np.where(ok, np.maximum(gap, g), gap)
    assert np.array_equal(want, gap <= 0)
    clear = np.abs(gap) > 1e-3 * extent
    print(f"away from contact: {clear.mean():.4f} of the pairs; intersecting: {got.mean():.3f}")
    assert clear.mean() > 0.97 and 0.2 < got.mean() < 0.8
    assert np.array_equal(got[clear], want[clear])


# ---- ABI ---------------------------------------------------------------------------------------------------
def test_record_layout_and_constants():
    assert C.sizeof(_lib.Tri) == 48
    t = _lib.Tri
    assert (t.v0.offset, t.pad0.offset, t.v1.offset, t.pad1.offset, t.v2.offset, t.pad2.offset) == (0, 12, 16, 28, 32, 44)
    assert (_lib.TRIS_COUNT, _lib.TRIS_ANY, _lib.TRIS_LIST, _lib.TRIS_PAD_SKIP_TRI) == (0, 1, 2, 1)
    res, args = SIGNATURE
    assert res is C.c_int32 and len(args) == 8
    assert len(_lib.SIGNATURES["bm_scene_overlap_triangles_counters"][1]) == 9
    assert {"bm_scene_overlap_triangles", "bm_scene_overlap_triangles_counters"} <= set(_lib.declared_symbols())


def test_null_scene_without_a_device():
    lib = _lib.load()
    out = (C.c_uint64 * 4)()
    bad = _lib.ERROR_INVALID_PARAMETER
    for mode in (0, 1, 2, 3):
        for flags in (0, 1, 2):
            assert lib.bm_scene_overlap_triangles(None, None, 0, mode, flags, None, None, None) == bad
            assert lib.bm_scene_overlap_triangles(None, None, 16, mode, flags, None, None, None) == bad
            assert lib.bm_scene_overlap_triangles_counters(None, None, 0, mode, flags, None, None, None, out) == bad
    assert lib.bm_scene_overlap_triangles_counters(None, None, 0, 0, 0, None, None, None, None) == bad


def test_cpp_layer_compiles_and_links(tmp_path):
    """IScene::overlapTriangles of include/beam/Beam.h compiles and links against the library."""
    src = tmp_path / "tris.cpp"
    src.write_text(SNIPPET)
    exe = tmp_path / "tris"
    subprocess.run(["g++", "-std=c++17", "-O1", "-I", os.path.join(REPO, "include"), str(src), "-o", str(exe),
                    _lib.LIB_PATH, f"-Wl,-rpath,{os.path.dirname(_lib.LIB_PATH)}"], check=True)
    assert exe.exists()


# ---- the traversal loses nothing: the node test walked over the oracle's BVH4 -------------------------------
def walk(rec, tris, a):
    """The query's traversal in numpy over exported BVH4 records (n, 32) and triangle records (ntri, 12) for the
    query triangle a (3, 3): a child is kept when ref != EMPTY_REF and, per axis, lo <= qhi and hi >= qlo — no
    arithmetic. Returns the global ids tri_tri accepts among the leaves reached (ascending) and the number of
    leaf triangles tested."""
    box = rec[:, :24].view(F).reshape(-1, 6, 4)
    ref = rec[:, 24:28]
    tf = tris.view(F)
    qlo, qhi = a.min(axis=0), a.max(axis=0)
    reached = []
    front = np.zeros(1 if tris.shape[0] else 0, np.int64)
    while front.size:
        b, r = box[front], ref[front]  # (m, 6, 4), (m, 4)
        with np.errstate(all="ignore"):
            keep = r != EMPTY_REF
            for k in range(3):
                keep &= (b[:, k, :] <= qhi[k]) & (b[:, 3 + k, :] >= qlo[k])
        kept = r[keep]
        leaves = kept[(kept & LEAF_BIT) != 0]
        front = kept[(kept & LEAF_BIT) == 0].astype(np.int64)
        for lf in leaves:
            first, cnt = int(lf & FIRST_MASK), int((lf >> 27) & 15) + 1
            reached.append(np.arange(first, first + cnt))
    at = np.concatenate(reached + [np.zeros(0, np.int64)]).astype(np.int64)
    t = tf[at]  # the leaf triangles reached, tested in one call
    v0 = t[:, 0:3]
    acc = tri_tri(a[0], a[1], a[2], v0, v0 + t[:, 4:7], v0 + t[:, 8:11])
    return np.sort(tris[at, 3][acc].astype(np.uint32)), at.size


def lemma_cases():
    out = []
    for shift in [(0, 0, 0)] + SHIFTS:
        verts, queries = suzanne_queries(shift, every=16)
        out.append((f"suzanne + {shift}", translated(scenes.load_mesh("suzanne"), shift), verts, queries))
    meshes = sliver_meshes()
    verts = tri_vertices(meshes)
    return out + [("slivers", meshes, verts, sliver_queries(verts))]


def test_the_node_test_reaches_every_accepted_triangle(oracle):
    for name, meshes, verts, queries in lemma_cases():
        rec, tris, _, _ = oracle.bvh_build(meshes, 4, width=4).export()
        assert rec.shape[1] == 32 and tris.shape[0] == verts.shape[0]
        # the premise: the reconstructed vertices lie inside their leaf's box
        assert leaf_boxes_hold_their_triangles(rec, tris) == verts.shape[0], name
        exp = brute_tris(queries, verts)
        assert exp["any"].any() and not exp["any"].all(), name
        tested = 0
        for i in range(queries.shape[0]):
            got, t = walk(rec, tris, queries[i])
            tested += t
            assert np.array_equal(got, exp["ids"][i]), (name, i)
        # and it does prune (the slivers all meet at the origin, and so do their boxes: there it prunes little)
        assert tested < (1.0 if name == "slivers" else 0.25) * queries.shape[0] * verts.shape[0], name
        lo, hi = verts.reshape(-1, 3).min(axis=0), verts.reshape(-1, 3).max(axis=0)
        whole, t = walk(rec, tris, np.stack([lo, hi, (lo + hi) * F(0.5)]))  # a query whose bounds hold the scene
        assert t == verts.shape[0], name


# ---- the designed query set --------------------------------------------------------------------------------
def test_designed_set_has_what_the_gpu_tests_need():
    verts, queries = suzanne_queries()
    assert verts.shape[0] == 15488 and queries.shape == (968, 3, 3)
    exp = brute_tris(queries, verts)
    cnt = exp["count"].astype(np.int64)
    print(f"second Suzanne, every 16th triangle: hit nothing {np.mean(cnt == 0):.3f}, one or more "
          f"{np.mean(cnt > 0):.3f}, largest {cnt.max()}, sum {cnt.sum()}")
    assert np.mean(cnt == 0) >= 0.25 and np.mean(cnt > 0) >= 0.25
