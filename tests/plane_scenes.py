"""Plane section queries (bm_scene_section_planes): the header's rule restated in numpy float32, the brute force
over all triangles, the generated closed meshes and the designed plane sets, shared by tests/test_planes_abi.py
(CPU) and tests/test_gpu_planes.py. Test infrastructure only.

The yardstick is brute_planes: plane_side below (s(x) of include/beam_c.h, one rounding per operation in the
order written) on every vertex of every triangle, read from the meshes' own vertex arrays through their index
triples, for every valid plane; the cut points by the header's two statements. No value in it comes from the
library.
"""
import numpy as np

F = np.float32
U = np.uint32


# ---- the rule (include/beam_c.h, "plane section queries") -------------------------------------------------
def plane_side(point, normal, x):
    """s(x) = (n.x*d.x + n.y*d.y) + n.z*d.z with d = x - point, float32 arrays (..., 3) that broadcast."""
    point, normal, x = (np.asarray(a, F) for a in (point, normal, x))
    with np.errstate(all="ignore"):
        d = x - point
        s = (normal[..., 0] * d[..., 0] + normal[..., 1] * d[..., 1]) + normal[..., 2] * d[..., 2]
    assert s.dtype == F
    return s


def valid_planes(points, normals):
    with np.errstate(all="ignore"):
        return np.isfinite(points).all(axis=1) & np.isfinite(normals).all(axis=1) & (normals != 0).any(axis=1)


def edge_cut(N, sN, P, sP):
    """The cut of edges with below ends N (s = sN < 0) and above ends P (s = sP >= 0): (m, 3) float32."""
    with np.errstate(all="ignore"):
        t = sN / (sN - sP)
        X = t[:, None] * P + (N - t[:, None] * N)
    assert X.dtype == F and t.dtype == F
    return X


def crossed(s):
    """s (..., 3): at least one vertex below (s < 0) and at least one above (not below)."""
    below = s < 0
    return below.any(axis=-1) & ~below.all(axis=-1)


def cut_segments(point, normal, tri):
    """(a, b) of crossed triangles tri (m, 3, 3) for one plane: a on the edge running from above to below, b on
    the edge running from below to above, going 0 -> 1 -> 2 -> 0."""
    tri = np.asarray(tri, F).reshape(-1, 3, 3)
    s = plane_side(point, normal, tri)
    below = s < 0
    assert crossed(s).all()
    rows = np.arange(tri.shape[0])
    nxt = np.array([1, 2, 0])
    b0, b1, b2 = below[:, 0], below[:, 1], below[:, 2]
    dn = np.where(~b0 & b1, 0, np.where(~b1 & b2, 1, 2))  # the down edge starts (above) at dn
    up = np.where(b0 & ~b1, 0, np.where(b1 & ~b2, 1, 2))  # the up edge starts (below) at up
    assert (~below[rows, dn] & below[rows, nxt[dn]]).all() and (below[rows, up] & ~below[rows, nxt[up]]).all()
    a = edge_cut(tri[rows, nxt[dn]], s[rows, nxt[dn]], tri[rows, dn], s[rows, dn])
    b = edge_cut(tri[rows, up], s[rows, up], tri[rows, nxt[up]], s[rows, nxt[up]])
    return a, b


def brute_planes(points, normals, verts):
    """What bm_scene_section_planes must find for planes (n,3)+(n,3) over the triangles verts (ntri,3,3) in
    global-id order (the meshes' own vertices): {"count": (n,) uint32, "any": (n,) bool, "ids": n ascending id
    arrays, "segs": n arrays (k, 8) uint32 — the bm_segment records (a, id, b, plane index) in ascending id}."""
    points, normals = np.asarray(points, F).reshape(-1, 3), np.asarray(normals, F).reshape(-1, 3)
    verts = np.asarray(verts, F).reshape(-1, 3, 3)
    n = points.shape[0]
    ids = [np.zeros(0, U) for _ in range(n)]
    segs = [np.zeros((0, 8), U) for _ in range(n)]
    if verts.shape[0]:
        for i in np.flatnonzero(valid_planes(points, normals)):
            g = np.flatnonzero(crossed(plane_side(points[i], normals[i], verts)))
            ids[i] = g.astype(U)
            if g.size:
                a, b = cut_segments(points[i], normals[i], verts[g])
                rec = np.zeros((g.size, 8), U)
                rec[:, 0:3], rec[:, 3], rec[:, 4:7], rec[:, 7] = a.view(U), g, b.view(U), i
                segs[i] = rec
    count = np.array([a.size for a in ids], U)
    return {"count": count, "any": count > 0, "ids": ids, "segs": segs}


def loop_closure(seg):
    """The a and the b of segment records (k, 8) uint32 are the same multiset of points, byte for byte."""
    a = np.ascontiguousarray(seg[:, 0:3])
    b = np.ascontiguousarray(seg[:, 4:7])
    key = lambda p: np.sort(p.view([("x", U), ("y", U), ("z", U)]).reshape(-1), order=("x", "y", "z"))
    return np.array_equal(key(a), key(b))


def tri_vertices(meshes):
    """(ntri, 3, 3) vertex positions by global triangle id (scene order, then face order)."""
    return np.concatenate([np.asarray(m["pos"], F).reshape(-1, 3)[np.asarray(m["idx"]).reshape(-1, 3)]
                           for m in meshes] + [np.zeros((0, 3, 3), F)])


def mesh(pos, idx):
    pos = np.ascontiguousarray(pos, F).reshape(-1, 3)
    return {"pos": pos, "nrm": np.tile(F([0, 0, 1]), (pos.shape[0], 1)), "idx": np.ascontiguousarray(idx, U).reshape(-1)}


def soup(verts):
    """One mesh of the triangles verts (ntri,3,3), unindexed: every vertex duplicated per triangle."""
    v = np.ascontiguousarray(verts, F).reshape(-1, 3)
    return [mesh(v, np.arange(v.shape[0], dtype=U))]


def translated(meshes, shift):
    return [dict(m, pos=np.asarray(m["pos"], F).reshape(-1, 3) + F(shift)) for m in meshes]


# ---- closed, consistently oriented meshes -------------------------------------------------------------------
def torus(nu=24, nv=16, R=2.0, r=0.75):
    """A welded torus about the z axis: nu * nv vertices, 2 * nu * nv triangles (768), outward winding. The
    vertex rows j = 0 (outer equator) and j = nv / 2 (inner equator) lie at z = 0 exactly, and the columns
    i = 0 and i = nu / 2 at y = 0."""
    u = 2 * np.pi * np.arange(nu) / nu
    v = 2 * np.pi * np.arange(nv) / nv
    snap = lambda a: np.where(np.abs(a) < 1e-12, 0.0, a)
    cu, su, cv, sv = snap(np.cos(u)), snap(np.sin(u)), snap(np.cos(v)), snap(np.sin(v))
    ring = R + r * cv
    pos = np.stack([cu[:, None] * ring[None, :], su[:, None] * ring[None, :], np.broadcast_to(r * sv, (nu, nv))], axis=-1)
    at = lambda i, j: (i % nu) * nv + (j % nv)
    idx = []
    for i in range(nu):
        for j in range(nv):
            a, b, c, d = at(i, j), at(i + 1, j), at(i + 1, j + 1), at(i, j + 1)
            idx += [a, b, c, a, c, d]
    return [mesh(pos.reshape(-1, 3), idx)]


def icosphere(levels=2, radius=1.5, centre=(0.25, -0.5, 0.125)):
    """An icosahedron subdivided `levels` times (320 triangles at 2), welded, outward winding."""
    t = (1 + 5 ** 0.5) / 2
    p = [(-1, t, 0), (1, t, 0), (-1, -t, 0), (1, -t, 0), (0, -1, t), (0, 1, t), (0, -1, -t), (0, 1, -t),
         (t, 0, -1), (t, 0, 1), (-t, 0, -1), (-t, 0, 1)]
    p = [np.asarray(q, np.float64) / np.linalg.norm(q) for q in p]
    f = [(0, 11, 5), (0, 5, 1), (0, 1, 7), (0, 7, 10), (0, 10, 11), (1, 5, 9), (5, 11, 4), (11, 10, 2), (10, 7, 6),
         (7, 1, 8), (3, 9, 4), (3, 4, 2), (3, 2, 6), (3, 6, 8), (3, 8, 9), (4, 9, 5), (2, 4, 11), (6, 2, 10),
         (8, 6, 7), (9, 8, 1)]
    for _ in range(levels):
        mid, nf = {}, []

        def m(a, b):
            k = (min(a, b), max(a, b))
            if k not in mid:
                q = p[a] + p[b]
                p.append(q / np.linalg.norm(q))
                mid[k] = len(p) - 1
            return mid[k]
        for a, b, c in f:
            ab, bc, ca = m(a, b), m(b, c), m(c, a)
            nf += [(a, ab, ca), (b, bc, ab), (c, ca, bc), (ab, bc, ca)]
        f = nf
    return [mesh(np.asarray(p) * radius + np.asarray(centre), np.asarray(f).reshape(-1))]


def closed_manifold(m):
    """Every directed edge of the mesh occurs once, and so does its reverse: closed, consistently oriented."""
    t = np.asarray(m["idx"]).reshape(-1, 3).astype(np.int64)
    e = np.concatenate([t[:, [0, 1]], t[:, [1, 2]], t[:, [2, 0]]])
    fwd = set(map(tuple, e.tolist()))
    return len(fwd) == e.shape[0] and all((b, a) in fwd for a, b in fwd)


# ---- the designed plane sets --------------------------------------------------------------------------------
SPECIAL_NORMALS = [(1, 0, 0), (0, -1, 0), (0, 0, 3), (-2, 0, 0), (0, 0.5, 0), (0, 0, -1), (1, 1, 0), (0, -2, 1),
                   (-1, 0, 0.5), (-0.0, 1, 0), (3, 0, -3), (0, 1e-3, 1e3)]


def designed_planes(verts, seed=11, rows=()):
    """(points, normals, groups) for the triangles verts: groups maps a name to the slice of its planes.
      random   12 planes through points of the bounding box, any orientation, normals of any length
      vertex   12 planes through a mesh vertex (that vertex is on the plane: s = 0 there, up to rounding of
               the other components' products, which is why the rule says which side it is)
      special  24: SPECIAL_NORMALS (axis-aligned and with zero components) through a box point, then through
               a mesh vertex
      miss     6 planes beyond the bounding box
      rows     the planes given by the caller (point, normal): those that contain a row of vertices"""
    rng = np.random.default_rng(seed)
    p = np.asarray(verts, F).reshape(-1, 3)
    lo, hi = p.min(axis=0).astype(np.float64), p.max(axis=0).astype(np.float64)
    pts, nrm, groups = [], [], {}

    def add(name, P, N):
        groups[name] = slice(len(pts), len(pts) + len(P))
        pts.extend(P)
        nrm.extend(N)
    unit = lambda k: rng.normal(size=(k, 3)) * 10 ** rng.uniform(-2, 2, (k, 1))
    add("random", rng.uniform(lo, hi, (12, 3)), unit(12))
    add("vertex", p[rng.integers(0, p.shape[0], 12)], unit(12))
    k = len(SPECIAL_NORMALS)
    add("special", np.concatenate([rng.uniform(lo, hi, (k, 3)), p[rng.integers(0, p.shape[0], k)]]),
        np.asarray(SPECIAL_NORMALS * 2, np.float64))
    d = rng.normal(size=(6, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    add("miss", (lo + hi) / 2 + d * np.linalg.norm(hi - lo) * rng.uniform(0.6, 3.0, (6, 1)), d * rng.choice([-1, 1], (6, 1)))
    if rows:
        add("rows", [r[0] for r in rows], [r[1] for r in rows])
    return np.ascontiguousarray(pts, F), np.ascontiguousarray(nrm, F), groups


TORUS_ROWS = [((0, 0, 0), (0, 0, 1)), ((5, -3, 0), (0, 0, -2)), ((0, 0, 0), (0, 1, 0)), ((0, 0, 0), (0, -1, 0)),
              ((0.5, 0, 0.25), (0, 4, 0)), ((0, 0, 0), (-0.0, 0, 1))]
INVALID = [([np.nan, 0, 0], [0, 0, 1]), ([0, np.inf, 0], [0, 0, 1]), ([0, 0, -np.inf], [0, 0, 1]),
           ([0, 0, 0], [np.nan, 0, 1]), ([0, 0, 0], [0, np.inf, 1]), ([0, 0, 0], [1, 0, -np.inf]),
           ([0, 0, 0], [0, 0, 0]), ([0, 0, 0], [-0.0, 0, -0.0]), ([np.nan] * 3, [np.nan] * 3)]


def torus_case():
    m = torus()
    verts = tri_vertices(m)
    return (m, verts) + designed_planes(verts, seed=11, rows=TORUS_ROWS)


def icosphere_case():
    m = icosphere()
    verts = tri_vertices(m)
    top = np.asarray(m[0]["pos"], F)[0]
    return (m, verts) + designed_planes(verts, seed=12, rows=[(top, (0, 0, 1)), (top, (1, 0, 0))])


# ---- the rules, by hand -------------------------------------------------------------------------------------
UP, DOWN = np.nextafter(F(0), F(1)), np.nextafter(F(0), F(-1))  # one ulp either side of zero
# (what, triangle, crossed) against the plane z = 0 with normal (0, 0, 1)
RULES = [
    ("a vertex on the plane, the others above", [[0, 0, 0], [1, 0, 1], [0, 1, 2]], False),
    ("a vertex on the plane, the others below", [[0.5, 0.25, 0], [1, 0, -1], [0, 1, -2]], True),
    ("an edge on the plane, the third above", [[0, 0, 0], [1, 0, 0], [0, 1, 2]], False),
    ("an edge on the plane, the third below", [[0, 0, 0], [1, 0, 0], [0, 1, -2]], True),
    ("in the plane", [[0, 0, 0], [1, 0, 0], [0, 1, 0]], False),
    ("in the plane, at minus zero", [[0, 0, -0.0], [1, 0, -0.0], [0, 1, 0]], False),
    ("one ulp above, the others above", [[0, 0, UP], [1, 0, 1], [0, 1, 2]], False),
    ("one ulp below, the others above", [[0, 0, DOWN], [1, 0, 1], [0, 1, 2]], True),
    ("one ulp above, the others below", [[0, 0, UP], [1, 0, -1], [0, 1, -2]], True),
    ("one ulp below, the others below", [[0, 0, DOWN], [1, 0, -1], [0, 1, -2]], False),
    ("straddling", [[0, 0, -1], [1, 0, 1], [0, 1, 3]], True),
    ("a point triangle on the plane", [[0.5, 0.5, 0]] * 3, False),
]
RULE_PLANE = (F([0, 0, 0]), F([0, 0, 1]))


def rule_scene():
    """The rule triangles as one scene (ids in RULES order), and the rule plane followed by the invalid ones."""
    verts = F([r[1] for r in RULES])
    pts = F([RULE_PLANE[0]] + [p[0] for p in INVALID])
    nrm = F([RULE_PLANE[1]] + [p[1] for p in INVALID])
    return verts, pts, nrm
