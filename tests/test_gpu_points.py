"""GPU checks of closest-point queries (bm_scene_closest_points).

The yardstick is tests/test_points_abi.py: the numpy float32 restatement of the header's triangle function,
evaluated over ALL triangles, the lexicographic minimum of (dd, id) under the rmax rule. The traversal prunes,
the brute force does not; t, u, v (as bit images) and tri_id must be equal. No expected value comes from the
library.
"""
from types import SimpleNamespace

import numpy as np
import pytest

from raytracercuda_amd import _lib, beam, scenes
from test_gpu_attrs import assert_rows, expected
from test_instances_abi import MIRROR, rotation, xform_mesh
from test_points_abi import NO_TRI, YARDSTICK_TOL_NO_SLIVERS, brute_force

pytestmark = pytest.mark.gpu

F = np.float32
MISS = np.uint32(NO_TRI)
QUAD_LDS = 24  # stack entries a query keeps in LDS (bm_trace_quad.h); beyond: the global overflow area
POS, NRM = beam.VERTEX_DATA_POSITION, beam.VERTEX_DATA_NORMAL
FACE, NORMALIZE = beam.ATTR_MESH_FACE, beam.ATTR_NORMALIZE


def bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


def tri_vertices(meshes):
    """(ntri, 3, 3) vertex positions by global triangle id (scene order, then face order)."""
    return np.concatenate([np.asarray(m["pos"], F).reshape(-1, 3)[np.asarray(m["idx"]).reshape(-1, 3)]
                           for m in meshes] + [np.zeros((0, 3, 3), F)])


def soup(verts):
    """One mesh of the triangles verts (ntri,3,3), unindexed."""
    v = np.ascontiguousarray(verts, F).reshape(-1, 3)
    return [{"pos": v, "nrm": np.tile(F([0, 0, 1]), (v.shape[0], 1)), "idx": np.arange(v.shape[0], dtype=np.uint32)}]


def build(ctx, meshes):
    scene = beam.IScene.create(ctx)
    keep = beam.upload_meshes(ctx, scene, meshes)
    scene.updateGPUScene()
    return scene, keep


def assert_records(res, exp, where=None, what=""):
    sel = slice(None) if where is None else where
    bad = res["tri_id"][sel] != exp["tri_id"][sel]
    assert not bad.any(), f"{what}: tri_id differs on {int(bad.sum())} points, first {np.flatnonzero(bad)[:5]}"
    for k in ("t", "u", "v"):
        assert np.array_equal(bits(res[k][sel]), bits(exp[k][sel])), (what, k)


def take(exp, idx):
    return {k: v[idx] for k, v in exp.items()}


def make_points(meshes, n, seed, near_only=False):
    """A third surface samples (barycentric samples of random faces, every eighth an exact vertex) moved along
    +- the face normal by 0, 1e-6, 1e-3 and 0.1 of the box diagonal; a third uniform in 1.5x the box; a third
    at 0.9-3 diagonals from the centre. near_only: the first third alone."""
    rng = np.random.default_rng(seed)
    verts = tri_vertices(meshes).astype(np.float64)
    lo, hi = verts.reshape(-1, 3).min(0), verts.reshape(-1, 3).max(0)
    c, diag = (lo + hi) / 2, float(np.linalg.norm(hi - lo))
    third = n // 3
    k = n - 2 * third
    f = rng.integers(0, verts.shape[0], k)
    a, b = rng.uniform(0, 1, k), rng.uniform(0, 1, k)
    flip = a + b > 1
    a[flip], b[flip] = 1 - a[flip], 1 - b[flip]
    corner = np.arange(k) % 8 == 0
    a[corner], b[corner] = rng.integers(0, 2, corner.sum()), 0.0
    v0, v1, v2 = verts[f, 0], verts[f, 1], verts[f, 2]
    nrm = np.cross(v1 - v0, v2 - v0)
    with np.errstate(all="ignore"):
        nrm = np.nan_to_num(nrm / np.linalg.norm(nrm, axis=1, keepdims=True))
    off = rng.choice([0.0, 1e-6, 1e-3, 0.1], k) * rng.choice([-1.0, 1.0], k) * diag
    near = v0 * (1 - a - b)[:, None] + v1 * a[:, None] + v2 * b[:, None] + nrm * off[:, None]
    if near_only:
        return F(near)
    inside = c + rng.uniform(-0.75, 0.75, (third, 3)) * (hi - lo)
    d = rng.normal(size=(third, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    far = c + d * rng.uniform(0.9, 3.0, (third, 1)) * diag
    return F(np.concatenate([near, inside, far]))


_CASES = {}


def case(ctx, name, n=3904):
    """Mesh, GPU scene, the point set and the brute force's answers for it — computed once per module run."""
    if name not in _CASES:
        meshes = scenes.load_mesh(name)
        scene, keep = build(ctx, meshes)
        pts = make_points(meshes, n, 7)
        verts = tri_vertices(meshes)
        exp = brute_force(pts, np.inf, verts)
        _CASES[name] = SimpleNamespace(meshes=meshes, scene=scene, keep=keep, pts=pts, verts=verts, exp=exp)
    return _CASES[name]


def teardown_module(module):
    for k in _CASES.values():
        k.scene.destroy()
    _CASES.clear()


# ---- 1. one triangle: every region ----------------------------------------------------------------------
def test_one_triangle_every_region(ctx):
    tri = F([[[0.25, -0.5, 1.0], [2.25, 0.0, 1.5], [0.75, 1.5, 0.5]]])
    v0, v1, v2 = tri[0].astype(np.float64)
    e1, e2 = v1 - v0, v2 - v0
    n = np.cross(e1, e2) / np.linalg.norm(np.cross(e1, e2))
    uv = [(-0.5, -0.5), (1.6, -0.3), (0.5, -0.7), (-0.3, 1.6), (-0.7, 0.5), (0.8, 0.8), (0.3, 0.3),  # regions 1..7
          (0, 0), (1, 0), (0, 1), (0.5, 0), (0, 0.5), (0.5, 0.5), (0.25, 0.25), (2.5, 2.5), (-3, 0.2)]
    pts = []
    for h in (0.0, 0.75, -2.0):
        pts += [v0 + e1 * a + e2 * b + n * h for a, b in uv]
    pts = F(pts)
    pts[7], pts[8], pts[9] = tri[0, 0], tri[0, 1], tri[0, 2]  # exactly on the vertices
    pts[10] = (tri[0, 0] + tri[0, 1]) * F(0.5)
    exp = brute_force(pts, np.inf, tri)
    assert set(exp["region"].tolist()) == set(range(1, 8)), sorted(set(exp["region"].tolist()))
    assert (exp["t"][7:10] == 0).all() and (exp["tri_id"] == 0).all()
    assert exp["t"][13] <= F(1e-6) and exp["t"][14] > 1  # in the interior; in the plane outside
    scene, keep = build(ctx, soup(tri))
    assert_records(scene.closestPoints(pts), exp, what="one triangle")
    scene.destroy()


# ---- 2. small scenes -----------------------------------------------------------------------------------
@pytest.mark.parametrize("ntri", [0, 2, 4, 5, 17])
def test_small_scenes(ctx, ntri):
    rng = np.random.default_rng(200 + ntri)
    base = rng.uniform(-1, 1, (ntri, 1, 3))
    verts = F(base + rng.uniform(-0.4, 0.4, (ntri, 3, 3)))
    scene, keep = build(ctx, soup(verts) if ntri else [])
    pts = F(rng.uniform(-2, 2, (203, 3)))
    res = scene.closestPoints(pts)
    if ntri == 0:  # a built scene with no triangles: all misses
        assert (res["tri_id"] == MISS).all() and np.isposinf(res["t"]).all()
        assert (bits(res["u"]) == 0).all() and (bits(res["v"]) == 0).all()
    else:
        exp = brute_force(pts, np.inf, verts)
        assert (exp["tri_id"] != MISS).all()
        assert_records(res, exp, what=f"{ntri} triangles")
    scene.destroy()


# ---- 3. meshes -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,n", [("suzanne", 3904), ("bunny", 1001)])
def test_meshes_against_brute_force(ctx, name, n):
    k = case(ctx, name, n)
    assert k.pts.shape[0] == n
    assert int((k.exp["tri_id"] == MISS).sum()) == 0
    assert len(set(k.exp["tri_id"].tolist())) > 100
    assert_records(k.scene.closestPoints(k.pts), k.exp, what=name)


# ---- 4. translated: where a relative-only pruning bound loses the winner -----------------------------
def test_translated_suzanne_near_surface(ctx):
    base = scenes.load_mesh("suzanne")
    moved = [dict(m, pos=np.asarray(m["pos"], F).reshape(-1, 3) + F([1000, -2000, 500])) for m in base]
    pts = make_points(moved, 3904, 7, near_only=True)
    assert pts.shape[0] == 3904 - 2 * (3904 // 3)
    verts = tri_vertices(moved)
    exp = brute_force(pts, np.inf, verts)
    assert (exp["tri_id"] != MISS).all() and len(set(exp["tri_id"].tolist())) > 100
    scene, keep = build(ctx, moved)
    assert_records(scene.closestPoints(pts), exp, what="translated suzanne")
    scene.destroy()


# ---- 5. ties -------------------------------------------------------------------------------------------
def test_ties_resolve_to_the_lowest_id(ctx):
    k = case(ctx, "suzanne")
    twice = k.meshes + k.meshes  # the same mesh as two plain entries
    scene, keep = build(ctx, twice)
    sel = np.arange(0, k.pts.shape[0], 6)
    res = scene.closestPoints(k.pts[sel])
    assert (res["tri_id"] < k.verts.shape[0]).all()
    assert_records(res, take(k.exp, sel), what="mesh added twice")  # the copy never wins: the single mesh's answers
    scene.destroy()
    # a point above the shared edge of two triangles
    quad = F([[[0, 0, 0], [1, 0, 0], [1, 1, 0]], [[0, 0, 0], [1, 1, 0], [0, 1, 0]]])
    pts = F([[0.5, 0.5, 1.0], [0.25, 0.25, -0.5], [0.75, 0.75, 0.0], [2.0, 2.0, 1.0], [-1.0, -1.0, 0.5]])
    for verts in (quad, quad[::-1]):
        exp = brute_force(pts, np.inf, verts)
        scene, keep = build(ctx, soup(verts))
        assert_records(scene.closestPoints(pts), exp, what="shared edge")
        scene.destroy()
    assert (brute_force(pts, np.inf, quad)["tri_id"] == 0).all()  # equal dd on the edge: the lowest id


# ---- 6. a degenerate triangle ----------------------------------------------------------------------------
def test_degenerate_triangle_counts_as_the_rule_says(ctx):
    verts = F([[[0, 0, 0], [1, 0, 0], [0, 1, 0]],
               [[2, 2, 2], [2, 2, 2], [2, 2, 2]],            # a point
               [[3, 0, 0], [5, 0, 0], [4, 0, 0]],            # collinear
               [[0, 3, 1], [0, 3.0000002, 1], [1e-7, 3, 1]],  # nearly a point
               [[-1, -1, -1], [-1, -1, -2], [-2, -1, -1]]])
    rng = np.random.default_rng(5)
    pts = F(np.concatenate([[[2.1, 2.2, 2.1], [4.0, 0.5, 0.1], [4.5, -0.25, 0.0], [6.0, 0.1, 0.0], [0.0, 3.1, 1.0],
                             [2, 2, 2], [4, 0, 0]], rng.uniform(-2, 6, (150, 3))]))
    exp = brute_force(pts, np.inf, verts)
    assert exp["tri_id"][0] == 1 and exp["region"][0] == 1  # the point triangle, through its vertex region
    scene, keep = build(ctx, soup(verts))
    assert_records(scene.closestPoints(pts), exp, what="degenerate")
    scene.destroy()


# ---- 7. rmax -------------------------------------------------------------------------------------------
def test_rmax_bounds_the_result(ctx):
    k = case(ctx, "suzanne")
    sel = np.arange(0, k.pts.shape[0], 16)
    t = k.exp["t"][sel]
    rmax = np.concatenate([t, np.nextafter(t, F(0)), t * F(0.5), np.full(sel.size, np.inf, F)])
    rmax = np.where(rmax > 0, rmax, F(1e-30))  # a point on the surface has t = 0: keep the point valid
    pts = np.tile(k.pts[sel], (4, 1))
    exp = brute_force(pts, rmax, k.verts)
    assert (exp["tri_id"] == MISS).any() and (exp["tri_id"][:sel.size] != MISS).sum() > sel.size // 2
    assert_records(take(exp, np.arange(3 * sel.size, 4 * sel.size)), take(k.exp, sel), what="rmax = inf")
    assert_records(k.scene.closestPoints(pts, rmax=rmax), exp, what="rmax")
    scalar = k.scene.closestPoints(k.pts[sel], rmax=0.05)
    assert_records(scalar, brute_force(k.pts[sel], F(0.05), k.verts), what="scalar rmax")


# ---- 8. invalid points ---------------------------------------------------------------------------------
def test_invalid_points_get_the_miss_record(ctx):
    k = case(ctx, "suzanne")
    n = 640
    pts, rmax = k.pts[:n].copy(), np.full(n, np.inf, F)
    sel = np.arange(3, n, 7)
    kind = (sel // 7) % 9
    for c in range(3):
        pts[sel[kind == c], c] = np.nan
        pts[sel[kind == 3 + c], c] = np.inf if c != 1 else -np.inf
    rmax[sel[kind == 6]] = np.nan
    rmax[sel[kind == 7]] = 0.0
    rmax[sel[kind == 8]] = -1.0
    invalid = np.zeros(n, bool)
    invalid[sel] = True
    res = k.scene.closestPoints(pts, rmax=rmax, counters=True)
    assert_records(res, take(k.exp, np.arange(n)), ~invalid, "neighbours of invalid points")
    assert (res["tri_id"][invalid] == MISS).all() and np.isposinf(res["t"][invalid]).all()
    assert (bits(res["u"][invalid]) == 0).all() and (bits(res["v"][invalid]) == 0).all()
    assert int(res["counters"][2]) == n - int(invalid.sum())
    alone = k.scene.closestPoints(pts[invalid], rmax=rmax[invalid], counters=True)
    assert [int(x) for x in alone["counters"]] == [0, 0, 0, 0]  # invalid points count nothing


# ---- 9. batch edges ------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 15, 16, 17, 63, 64, 65])
def test_batch_edges_write_nothing_past_n(ctx, n):
    import torch
    k = case(ctx, "suzanne")
    dev = torch.device("cuda", ctx.device)
    packed = np.zeros((n, 4), F)
    packed[:, 0:3], packed[:, 3] = k.pts[:n], np.inf
    hits = torch.full((n + 64, 4), -7.5, dtype=torch.float32, device=dev)
    p_dev = torch.from_numpy(packed).to(dev)
    torch.cuda.synchronize()
    assert k.scene.closestPointsDevice(p_dev.data_ptr(), n, hits.data_ptr()) == 0
    ctx.sync()
    h = hits.cpu().numpy()
    assert np.all(h[n:] == F(-7.5))
    got = {"t": h[:n, 0], "u": h[:n, 1], "v": h[:n, 2], "tri_id": h.view(np.uint32)[:n, 3]}
    assert_records(got, take(k.exp, np.arange(n)), what=f"n = {n}")


def test_small_grid_strides_over_the_batches(ctx):
    k = case(ctx, "suzanne")
    small = beam.Context(device=0, params={"trace_grid": 2})  # 8 waves: about 30 batches each
    scene, keep = build(small, k.meshes)
    assert_records(scene.closestPoints(k.pts), k.exp, what="two workgroups")
    scene.destroy()
    small.close()


# ---- 10. the stack's overflow area ---------------------------------------------------------------------
def deep_scene():
    """Centres whose 30-bit Morton keys are 0, every single bit 2^k (five triangles each, so the chain's
    siblings are internal nodes and every BVH4 record on it has four children) and the all-ones key: the
    Karras tree is a chain towards key 0, and a query from beyond the origin corner finds the chain nearest
    at every record, so it keeps pushing siblings until its first leaf."""
    h = 0.125
    shape = np.array([[-h, -h, -h], [h, h, h], [h, -h, 0.0]])  # its AABB is centre +- h
    centres = [np.zeros(3), np.full(3, 1024.0)]
    for axis in range(3):
        for j in range(10):
            c = np.full(3, 0.25)
            c[axis] = 2.0 ** j + 0.5
            centres += [c] * 5
    return F(np.asarray(centres)[:, None, :] + shape[None, :, :])


def test_deep_descent_uses_the_overflow_area(ctx):
    verts = deep_scene()
    rng = np.random.default_rng(9)
    outside = F(np.concatenate([-rng.uniform(50, 400, (40, 3)), [[-100, -100, -100], [-1, -2, -3]],
                                rng.uniform(-10, 1100, (30, 3))]))
    exp = brute_force(outside, np.inf, verts)
    assert exp["tri_id"][40] == 0  # the triangle in the origin corner
    scene, keep = build(ctx, soup(verts))
    res = scene.closestPoints(outside, counters=True)
    deepest = int(res["counters"][3])
    print(f"deep scene: {verts.shape[0]} triangles, deepest stack {deepest} entries (LDS holds {QUAD_LDS})")
    assert deepest > QUAD_LDS, f"the overflow path did not run: deepest stack {deepest} <= {QUAD_LDS}"
    assert_records(res, exp, what="deep scene, counting kernel")
    assert_records(scene.closestPoints(outside), exp, what="deep scene")
    scene.destroy()


# ---- 11. counters --------------------------------------------------------------------------------------
def test_counters(ctx):
    k = case(ctx, "suzanne")
    n, ntri = k.pts.shape[0], k.verts.shape[0]
    res = k.scene.closestPoints(k.pts, counters=True)
    assert_records(res, k.exp, what="counting kernel")
    nodes, tris, found, deepest = (int(x) for x in res["counters"])
    print(f"suzanne, {n} points: {nodes / n:.1f} node records and {tris / n:.1f} triangle evaluations per point, "
          f"deepest stack {deepest}")
    assert found == int((k.exp["tri_id"] != MISS).sum()) == n
    assert nodes > 0 and deepest > 0
    assert tris <= 0.05 * n * ntri, (tris, n * ntri)  # pruning works at all (a condition, not a measurement)


# ---- 12. refit -----------------------------------------------------------------------------------------
def test_query_after_refit(ctx):
    k = case(ctx, "suzanne")
    scene = beam.IScene.create(ctx)
    meshes = beam.upload_meshes(ctx, scene, k.meshes)
    scene.updateGPUScene()
    moved = []
    for m in k.meshes:  # scaled and sheared
        p = np.asarray(m["pos"], F).reshape(-1, 3)
        q = p.copy()
        q[:, 0] = p[:, 0] * F(1.25) + p[:, 1] * F(0.5)
        q[:, 1] = p[:, 1] * F(0.75)
        q[:, 2] = p[:, 2] * F(1.5) + p[:, 0] * F(0.25)
        moved.append(dict(m, pos=q))
    for m, mv in zip(meshes, moved):
        assert m.setVertexData(mv["pos"], mv["pos"].shape[0], 3, POS) == 0
    scene.refitGPUScene()
    pts = make_points(moved, 900, 21)
    exp = brute_force(pts, np.inf, tri_vertices(moved))
    assert (exp["tri_id"] != MISS).all()
    assert_records(scene.closestPoints(pts), exp, what="after refit")
    scene.destroy()


# ---- 13. instances and hit attributes ------------------------------------------------------------------
def test_instances_and_hit_attributes(ctx):
    k = case(ctx, "suzanne")
    base = k.meshes[0]
    x_rot = rotation((1, 2, 3), 0.7, (3.5, -0.25, 2.0))
    x_mir = np.array(MIRROR, F)
    x_mir[:, 3] = F([-3.25, 0.5, -1.0])
    scene = beam.IScene.create(ctx)
    mesh = beam.upload_meshes(ctx, scene, [base])[0]  # entry 0: the plain one
    assert scene.addInstance(mesh, x_rot) == 1
    assert scene.addInstance(mesh, x_mir) == 2
    scene.updateGPUScene()
    pre = [base, xform_mesh(x_rot, base), xform_mesh(x_mir, base)]  # the header's transform arithmetic, restated
    pts = make_points(pre, 900, 33)
    exp = brute_force(pts, np.inf, tri_vertices(pre))
    ntri = k.verts.shape[0]
    assert set((exp["tri_id"] // ntri).tolist()) == {0, 1, 2}
    res = scene.closestPoints(pts)
    assert_records(res, exp, what="instances")
    hits = np.zeros((pts.shape[0], 4), F)
    hits[:, 0], hits[:, 1], hits[:, 2] = res["t"], res["u"], res["v"]
    hits.view(np.uint32)[:, 3] = res["tri_id"]
    pos, face = scene.hitAttributes(hits, [(POS, 3), (FACE, 2)])
    assert_rows(pos, expected(pre, hits, POS, 3), "closest point")
    assert_rows(face, expected(pre, hits, FACE, 2), "owner")
    assert np.array_equal(face[:, 0], (exp["tri_id"] // ntri).astype(np.int32))  # m is the entry index
    scene.destroy()


# ---- 14. chaining on the device ------------------------------------------------------------------------
def test_torch_chain_into_hit_attributes(ctx):
    import torch
    k = case(ctx, "suzanne")
    dev = torch.device("cuda", 0)
    tctx = beam.Context(device=0, stream=torch.cuda.current_stream(dev).cuda_stream)
    scene, keep = build(tctx, k.meshes)
    n = k.pts.shape[0]
    pts = torch.from_numpy(k.pts).to(dev)
    # no synchronisation from here to the end of the chain
    res = scene.closestPoints(pts)
    assert res["hits"].is_cuda and res["hits"].shape == (n, 4) and res["tri_id"].dtype == torch.int32
    pos, nrm = scene.hitAttributes(res["hits"], [(POS, 3), (NRM, 3, NORMALIZE)])
    gap = torch.linalg.vector_norm(pos.double() - pts.double(), dim=1)
    packed = torch.cat([pts, torch.full((n, 1), float("inf"), device=dev)], dim=1).contiguous()
    again = scene.closestPoints(packed)
    bounded = scene.closestPoints(pts, rmax=res["t"] * 0.5 + 1e-30)
    torch.cuda.synchronize()
    hits = res["hits"].cpu().numpy()
    got = {"t": hits[:, 0], "u": hits[:, 1], "v": hits[:, 2], "tri_id": hits.view(np.uint32)[:, 3]}
    assert_records(got, k.exp, what="torch path")
    assert torch.equal(again["hits"].view(torch.int32), res["hits"].view(torch.int32))
    assert_rows(pos.cpu().numpy(), expected(k.meshes, hits, POS, 3), "closest point")
    assert_rows(nrm.cpu().numpy(), expected(k.meshes, hits, NRM, 3, NORMALIZE), "normal there")
    # the interpolated position lies at distance t from the point, within the yardstick's own error
    scale = float(np.abs(k.pts).max() + np.abs(k.verts).max())
    worst = float(np.abs(gap.cpu().numpy() - k.exp["t"].astype(np.float64)).max())
    print(f"chain: largest | |position - p| - t | = {worst / (2.0 ** -24 * scale):.2f} x 2^-24 x scale ({scale:.3g})")
    assert worst <= YARDSTICK_TOL_NO_SLIVERS * 2.0 ** -24 * scale
    far = bounded["tri_id"].cpu().numpy()
    assert (far[k.exp["t"] > 0] == -1).all()  # nothing within half the distance
    scene.destroy()
    tctx.close()


# ---- 15. errors ----------------------------------------------------------------------------------------
def test_errors(ctx):
    import torch
    k = case(ctx, "suzanne")
    dev = torch.device("cuda", ctx.device)
    n = 64
    pts = torch.zeros((n + 1, 4), dtype=torch.float32, device=dev)
    out = torch.zeros((n + 1, 4), dtype=torch.float32, device=dev)
    torch.cuda.synchronize()
    pp, op = pts.data_ptr(), out.data_ptr()
    bad = _lib.ERROR_INVALID_PARAMETER
    unbuilt = beam.IScene.create(ctx)
    assert unbuilt.closestPointsDevice(pp, n, op) == _lib.ERROR_NOT_BUILT
    unbuilt.destroy()
    s = k.scene
    assert s.closestPointsDevice(pp, n, op) == 0
    assert s.closestPointsDevice(0, n, op) == bad and s.closestPointsDevice(pp, n, 0) == bad
    assert s.closestPointsDevice(0, 0, 0) == 0  # n = 0: nothing to read or write
    off_p, off_o = pts.view(-1)[1:].data_ptr(), out.view(-1)[1:].data_ptr()  # 4 bytes in
    assert off_p == pp + 4 and off_o == op + 4
    assert s.closestPointsDevice(off_p, n, op) == bad and s.closestPointsDevice(pp, n, off_o) == bad
    cnt = np.zeros(4, np.uint64)
    for flags in (1, 2, 0x80000000):  # no flag bits are defined
        assert s.closestPointsDevice(pp, n, op, flags=flags) == bad
        assert s.closestPointsDevice(pp, n, op, counters=cnt, flags=flags) == bad
    assert s.ctx.lib.bm_scene_closest_points_counters(s.h, pp, n, 0, op, None) == bad
    ctx.sync()
    tiny = [{"pos": F([[0, 0, 1], [1, 0, 1], [0, 1, 1]]), "nrm": F([[0, 0, 1]] * 3), "idx": np.uint32([0, 1, 2])}]
    for kw in ({"reference_kd": True}, {"reference_hash": True}, {"bvh_width": 2}):
        other = beam.Context(device=0, **kw)
        sc, keep = build(other, tiny)
        assert sc.closestPointsDevice(pp, n, op) == bad, kw
        assert sc.closestPointsDevice(pp, n, op, counters=cnt) == bad, kw
        sc.destroy()
        other.close()


def test_repeated_device_context_queries_on_the_root(ctx):
    k = case(ctx, "suzanne")
    multi = beam.Context(devices=[0, 0])
    scene, keep = build(multi, k.meshes)
    assert_records(scene.closestPoints(k.pts), k.exp, what="devices=[0, 0]")
    scene.destroy()
    multi.close()
