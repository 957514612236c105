"""GPU checks of multi-result point queries (bm_scene_closest_points_multi): the k nearest triangles per point
and the number of triangles within rmax.

Every comparison is bit-exact against brute_points_multi of tests/test_points_multi_abi.py: the header's triangle
function restated in numpy float32, evaluated for every triangle and every point, sorted by (dd, id). The
traversal prunes, the brute force does not. A reference is computed once per scene with k = 16 and left
unchanged: a smaller k expects its first k columns. No expected value comes from the library.
"""
from types import SimpleNamespace

import numpy as np
import pytest

import deep_scenes as ds
from raytracercuda_amd import _lib, beam, scenes
from test_points_abi import YARDSTICK_TOL_NO_SLIVERS
from test_points_multi_abi import (F, KMAX, NO_TRI, SHARED_EDGE, SHARED_EDGE_POINTS, TIE_COLUMNS, bits,
                                   brute_points_multi, check_runs, radius_set, radius_subset, suzanne_points,
                                   tie_points, tri_vertices, RADIUS_COLUMNS)

pytestmark = pytest.mark.gpu

ALL = _lib.MULTI_COUNT_ALL
BAD = _lib.ERROR_INVALID_PARAMETER
QUAD_LDS = 24  # stack entries a query keeps in LDS (bm_trace_quad.h); beyond: the global overflow area
POS = beam.VERTEX_DATA_POSITION


def soup(verts):
    """One mesh of the triangles verts (ntri,3,3), unindexed."""
    v = np.ascontiguousarray(verts, F).reshape(-1, 3)
    return [{"pos": v, "nrm": np.tile(F([0, 0, 1]), (v.shape[0], 1)), "idx": np.arange(v.shape[0], dtype=np.uint32)}]


def build(ctx, meshes):
    scene = beam.IScene.create(ctx)
    keep = beam.upload_meshes(ctx, scene, meshes)
    scene.updateGPUScene()
    return scene, keep


def frozen(res):
    for a in res.values():
        a.setflags(write=False)
    return res


def assert_multi(res, exp, k, count_all=False, what=""):
    """res (k records per point) equals the first k columns of exp (brute_points_multi with at least k columns,
    the same points and rmax), counts included."""
    assert res["tri_id"].shape[1] == k
    bad = (res["tri_id"] != exp["tri_id"][:, :k]).any(axis=1)
    assert not bad.any(), f"{what}: tri_id differs on {int(bad.sum())} points, first {np.flatnonzero(bad)[:5]}"
    for key in ("t", "u", "v"):
        assert np.array_equal(bits(res[key]), bits(exp[key][:, :k])), (what, key)
    want = exp["total"] if count_all else np.minimum(exp["total"], np.uint32(k))
    assert np.array_equal(res["count"], want), (what, "count")


def both(scene, pts, exp, ks, rmax=None, what=""):
    for k in ks:
        for count_all in (False, True):
            res = scene.closestPointsMulti(pts, rmax=rmax, k=k, count_all=count_all)
            assert_multi(res, exp, k, count_all, f"{what}, k = {k}, count_all = {count_all}")


_CASES = {}


def case(ctx, name):
    """Meshes, GPU scene, points and brute_points_multi's k = 16 answer (rmax = inf) — made once per module run.
    suzanne: tests/test_gpu_points.py's 3,904 points; bunny: its 1,001; suzanne3 / suzanne6: the mesh added
    three / six times (ids g, g + N, ...: bit-equal dd) with tie_points(), 18 columns."""
    if name not in _CASES:
        from test_gpu_points import make_points
        copies = {"suzanne3": 3, "suzanne6": 6}.get(name, 1)
        one = scenes.load_mesh("suzanne" if copies > 1 else name)
        meshes = one * copies
        if copies > 1:
            pts, cols = tie_points(), TIE_COLUMNS
        else:
            pts, cols = (suzanne_points() if name == "suzanne" else make_points(one, 1001, 7)), KMAX
        verts = tri_vertices(meshes)
        scene, keep = build(ctx, meshes)
        exp = brute_points_multi(pts, np.inf, verts, cols)
        _CASES[name] = SimpleNamespace(meshes=meshes, verts=verts, scene=scene, keep=keep, pts=pts, exp=frozen(exp))
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
    pts = F([v0 + e1 * a + e2 * b + n * h for h in (0.0, 0.75, -2.0) for a, b in uv])
    pts[7], pts[8], pts[9] = tri[0, 0], tri[0, 1], tri[0, 2]  # exactly on the vertices
    from test_points_abi import brute_force
    assert set(brute_force(pts, np.inf, tri)["region"].tolist()) == set(range(1, 8))
    exp = brute_points_multi(pts, np.inf, tri, KMAX)
    assert (exp["total"] == 1).all() and (exp["tri_id"][:, 0] == 0).all() and (exp["tri_id"][:, 1:] == NO_TRI).all()
    scene, keep = build(ctx, soup(tri))
    both(scene, pts, exp, (1, 4, 16), what="one triangle")
    rmax = np.where(np.arange(pts.shape[0]) % 2 == 0, exp["t"][:, 0], exp["t"][:, 0] * F(0.5))
    rmax = np.where(rmax > 0, rmax, F(1e-30))
    bounded = brute_points_multi(pts, rmax, tri, KMAX)
    assert 0 < int(bounded["total"].sum()) < pts.shape[0]
    both(scene, pts, bounded, (1, 4, 16), rmax=rmax, what="one triangle, rmax")
    scene.destroy()


# ---- 2. tiny scenes: the empty tree, one leaf, a full leaf, a leaf plus one, several records ----------------
@pytest.mark.parametrize("ntri", [0, 2, 4, 5, 17])
def test_tiny_scenes(ctx, ntri):
    rng = np.random.default_rng(200 + ntri)
    base = rng.uniform(-1, 1, (ntri, 1, 3))
    verts = F(base + rng.uniform(-0.4, 0.4, (ntri, 3, 3)))
    scene, keep = build(ctx, soup(verts) if ntri else [])
    pts = F(rng.uniform(-2, 2, (203, 3)))
    for rmax in (None, F(1.25)):
        exp = brute_points_multi(pts, np.inf if rmax is None else rmax, verts, KMAX)
        if ntri:
            assert (exp["total"] == ntri).all() if rmax is None else 0 < int(exp["total"].sum()) < ntri * 203
        both(scene, pts, exp, (1, 2, 4, 5, 16), rmax=rmax, what=f"{ntri} triangles")
        res = scene.closestPointsMulti(pts, rmax=rmax, k=0, count_all=True, counters=True)
        assert res["t"].shape == (203, 0) and np.array_equal(res["count"], exp["total"])
        assert int(res["counters"][2]) == int(exp["total"].sum())
        if ntri == 0:  # a built scene with no triangles: all misses, nothing evaluated
            assert int(res["counters"][1]) == 0 and (exp["total"] == 0).all()
    scene.destroy()


# ---- 3. meshes -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [1, 3, 4, 5, 16])
def test_suzanne(ctx, k):
    c = case(ctx, "suzanne")
    assert c.pts.shape[0] == 3904 and (c.exp["total"] > KMAX).all()
    assert len(set(c.exp["tri_id"][:, 0].tolist())) > 100
    both(c.scene, c.pts, c.exp, (k,), what="suzanne")


def test_suzanne_agrees_with_the_single_result_query(ctx):
    c = case(ctx, "suzanne")
    single = c.scene.closestPoints(c.pts, counters=True)
    r1 = c.scene.closestPointsMulti(c.pts, k=1, counters=True)
    r4 = c.scene.closestPointsMulti(c.pts, k=4, counters=True)
    r16 = c.scene.closestPointsMulti(c.pts, k=16, counters=True)
    a16 = c.scene.closestPointsMulti(c.pts, k=16, count_all=True, counters=True)
    for r in (r1, r4, r16, a16):  # record 0 is the single-result query's record, bit for bit
        assert np.array_equal(r["tri_id"][:, 0], single["tri_id"])
        for key in ("t", "u", "v"):
            assert np.array_equal(bits(r[key][:, 0]), bits(single[key])), key
    # k = 1 without the flag is quad_nearest's sequence of visits and leaf evaluations
    assert int(r1["counters"][0]) == int(single["counters"][0]) and int(r1["counters"][1]) == int(single["counters"][1])
    assert int(r1["counters"][2]) == int(single["counters"][2]) == c.pts.shape[0]
    assert int(r1["counters"][3]) == int(single["counters"][3])
    n = c.pts.shape[0]
    print("suzanne, per point: " + ", ".join(f"{name} {int(r['counters'][0]) / n:.1f} node records, "
                                             f"{int(r['counters'][1]) / n:.1f} triangle evaluations"
                                             for name, r in (("k=1", r1), ("k=4", r4), ("k=16", r16), ("all", a16))))
    assert int(r16["counters"][0]) >= int(r4["counters"][0]) >= int(r1["counters"][0])
    assert int(r16["counters"][1]) >= int(r4["counters"][1]) >= int(r1["counters"][1])
    assert int(r16["counters"][2]) == 16 * n and int(r4["counters"][2]) == 4 * n
    assert int(a16["counters"][2]) == int(c.exp["total"].sum()) == int(a16["count"].sum())  # rmax = inf: everything
    assert int(a16["counters"][1]) == n * c.verts.shape[0]


@pytest.mark.parametrize("k", [4, 16])
def test_bunny(ctx, k):
    c = case(ctx, "bunny")
    assert c.pts.shape[0] == 1001
    both(c.scene, c.pts, c.exp, (k,), what="bunny")


# ---- 4. radius sets: every relation between |N| and k ------------------------------------------------------
@pytest.mark.parametrize("k", [4, 16])
def test_radius_sets(ctx, k):
    import torch
    c = case(ctx, "suzanne")
    pts = radius_subset()
    ranked = brute_points_multi(pts, np.inf, c.verts, RADIUS_COLUMNS)
    rmax, js = radius_set(ranked["dd"], k)
    exp = brute_points_multi(pts, rmax, c.verts, KMAX)
    tot = exp["total"].astype(np.int64)
    for name, m in (("|N| = 0", tot == 0), ("0 < |N| < k", (tot > 0) & (tot < k)), ("|N| = k", tot == k),
                    ("|N| > k", tot > k), ("|N| > 16", tot > 16)):
        assert m.mean() >= 0.10, (name, float(m.mean()))
    both(c.scene, pts, exp, (k,), rmax=rmax, what="radius set")
    res = c.scene.closestPointsMulti(pts, rmax=rmax, k=0, count_all=True, counters=True)
    assert np.array_equal(res["count"], exp["total"]) and int(res["counters"][2]) == int(tot.sum())
    # the pure count through the raw call: a NULL hits_dev, nothing written beside the counts
    dev = torch.device("cuda", ctx.device)
    n = pts.shape[0]
    packed = np.zeros((n, 4), F)
    packed[:, 0:3], packed[:, 3] = pts, rmax
    p_dev = torch.from_numpy(packed).to(dev)
    counts = torch.full((n + 64,), -3, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    assert c.scene.closestPointsMultiDevice(p_dev.data_ptr(), n, 0, 0, counts.data_ptr(), ALL) == 0
    ctx.sync()
    got = counts.cpu().numpy()
    assert np.array_equal(got[:n].view(np.uint32), exp["total"]) and np.all(got[n:] == -3)


# ---- 5. ties at the list's edge --------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["suzanne3", "suzanne6"])
def test_ties_resolve_to_the_lowest_ids(ctx, name):
    c = case(ctx, name)
    copies = int(name[-1])
    check_runs(c.exp, copies, c.verts.shape[0] // copies)
    for k in (4, 5, 16):  # the reference itself: the list ends inside a run of equal dd
        inside = (c.exp["dd"][:, k - 1] == c.exp["dd"][:, k]) & (c.exp["tri_id"][:, k - 1] < c.exp["tri_id"][:, k])
        assert inside.mean() >= 0.5, (k, float(inside.mean()))
    both(c.scene, c.pts, c.exp, (1, 4, 5, 16), what=name)


def test_shared_edge(ctx):
    for verts in (SHARED_EDGE, SHARED_EDGE[::-1]):
        exp = brute_points_multi(SHARED_EDGE_POINTS, np.inf, verts, KMAX)
        assert (exp["dd"][:, 0] == exp["dd"][:, 1]).sum() >= 4
        scene, keep = build(ctx, soup(verts))
        both(scene, SHARED_EDGE_POINTS, exp, (1, 2, 3, 4), what="shared edge")
        scene.destroy()


def test_distances_that_overflow_tie_at_infinity(ctx):
    """Points so far away that every squared distance, and every squared box distance, overflows to +inf. By the
    definition inf <= rmax*rmax = inf holds, so all triangles are in N, tied, in id order, with t = +inf. A
    stack entry's key then equals the bound (+inf both): this is where a pop that drops `key >= bound` instead of
    `key > bound` loses every subtree but the first. The last point's distances stay finite and tie by rounding."""
    rng = np.random.default_rng(217)
    verts = F(rng.uniform(-1, 1, (17, 1, 3)) + rng.uniform(-0.4, 0.4, (17, 3, 3)))
    pts = F([[1e20, -2e20, 3e19], [-3e25, 1e22, 1e21], [0, 0, 5e19], [1e19, 1e19, 1e19]])
    exp = brute_points_multi(pts, np.inf, verts, KMAX)
    assert (exp["total"] == 17).all() and np.isposinf(exp["t"][:3]).all() and np.isfinite(exp["t"][3]).all()
    assert (exp["tri_id"] == np.arange(16)).all()
    scene, keep = build(ctx, soup(verts))
    both(scene, pts, exp, (1, 4, 5, 16), what="overflowing distances")
    single = scene.closestPoints(pts)
    assert np.array_equal(single["tri_id"], exp["tri_id"][:, 0]) and np.array_equal(bits(single["t"]), bits(exp["t"][:, 0]))
    scene.destroy()


# ---- 6. translated: bit-exactness at large coordinates ---------------------------------------------------
@pytest.mark.parametrize("shift", [(1000, -2000, 500), (65536, 0, 0)])
def test_translated_suzanne_near_surface(ctx, shift):
    """Suzanne translated by (1000, -2000, 500), and along x alone by 65,536 (there the box padding across y and
    z is the smallest the build makes against the largest coordinate), with tests/test_gpu_points.py's 1,302
    near-surface points: the coordinates are a thousand times the distances and more, so every rounding of the
    triangle function and of the box distance is large against dd. What this checks is that lists and counts stay bit-equal to the brute force
    there, at k = 1 (the smallest dd as the bound) and k = 4. It does not tell an absolute pruning margin from
    a relative one: a trial build with the margin replaced by the factor 1 + 2^-18 passes it, because the
    build pads every box by 2^-20 of the scene's extent and more."""
    from test_gpu_points import make_points
    base = scenes.load_mesh("suzanne")
    moved = [dict(m, pos=np.asarray(m["pos"], F).reshape(-1, 3) + F(shift)) for m in base]
    pts = make_points(moved, 3904, 7, near_only=True)
    assert pts.shape[0] == 1302
    verts = tri_vertices(moved)
    exp = brute_points_multi(pts, np.inf, verts, KMAX)
    assert len(set(exp["tri_id"][:, 0].tolist())) > 100
    scene, keep = build(ctx, moved)
    both(scene, pts, exp, (1, 4), what="translated suzanne")
    rmax = np.where(np.arange(pts.shape[0]) % 2 == 0, exp["t"][:, 3], np.nextafter(exp["t"][:, 3], F(0)))
    rmax = np.where(rmax > 0, rmax, F(1e-30))
    both(scene, pts, brute_points_multi(pts, rmax, verts, KMAX), (1, 4), rmax=rmax, what="translated suzanne, rmax")
    scene.destroy()


# ---- 7. degenerate triangles -----------------------------------------------------------------------------
def test_degenerate_triangles_are_neither_listed_nor_counted(ctx):
    verts = F([[[0, 0, 0], [1, 0, 0], [0, 1, 0]],
               [[2, 2, 2], [2, 2, 2], [2, 2, 2]],            # a point
               [[3, 0, 0], [3, 0, 0], [5, 0, 0]],            # v1 = v0: NaN beside its vertex regions
               [[3, 0, 0], [5, 0, 0], [4, 0, 0]],            # collinear
               [[0, 3, 1], [0, 3.0000002, 1], [1e-7, 3, 1]],  # nearly a point
               [[-1, -1, -1], [-1, -1, -2], [-2, -1, -1]]])
    rng = np.random.default_rng(5)
    pts = F(np.concatenate([[[2.1, 2.2, 2.1], [4.0, 0.5, 0.1], [4.5, -0.25, 0.0], [6.0, 0.1, 0.0], [0.0, 3.1, 1.0],
                             [2, 2, 2], [4, 0, 0]], rng.uniform(-2, 6, (150, 3))]))
    exp = brute_points_multi(pts, np.inf, verts, KMAX)
    assert 0 < int((exp["total"] < verts.shape[0]).sum()) < pts.shape[0]  # a NaN dd on some points, not on all
    assert (exp["total"] >= verts.shape[0] - 1).all()
    scene, keep = build(ctx, soup(verts))
    both(scene, pts, exp, (1, 4, 16), what="degenerate")
    res = scene.closestPointsMulti(pts, k=0, count_all=True)
    assert np.array_equal(res["count"], exp["total"])
    scene.destroy()


# ---- 8. invalid points -----------------------------------------------------------------------------------
def test_invalid_points_get_miss_records(ctx):
    c = case(ctx, "suzanne")
    n = 640
    pts, rmax = c.pts[:n].copy(), np.full(n, np.inf, F)
    sel = np.arange(3, n, 7)
    kind = (sel // 7) % 9
    for ax in range(3):
        pts[sel[kind == ax], ax] = np.nan
        pts[sel[kind == 3 + ax], ax] = np.inf if ax != 1 else -np.inf
    rmax[sel[kind == 6]] = np.nan
    rmax[sel[kind == 7]] = 0.0
    rmax[sel[kind == 8]] = -1.0
    invalid = np.zeros(n, bool)
    invalid[sel] = True
    exp = {key: val[:n].copy() for key, val in c.exp.items()}
    exp["t"][invalid], exp["u"][invalid], exp["v"][invalid] = np.inf, 0, 0
    exp["tri_id"][invalid], exp["total"][invalid] = NO_TRI, 0
    again = brute_points_multi(pts, rmax, c.verts, 1)  # the brute force's own rule, on k = 1
    assert np.array_equal(again["tri_id"][:, 0], exp["tri_id"][:, 0]) and np.array_equal(again["total"], exp["total"])
    for k, count_all in ((1, False), (5, False), (16, False), (16, True), (0, True)):
        res = c.scene.closestPointsMulti(pts, rmax=rmax, k=k, count_all=count_all, counters=True)
        assert_multi(res, exp, k, count_all, "invalid points")
        assert (res["count"][invalid] == 0).all()
        assert int(res["counters"][2]) == int(res["count"].sum())
    alone = c.scene.closestPointsMulti(pts[invalid], rmax=rmax[invalid], k=4, counters=True)
    assert [int(x) for x in alone["counters"]] == [0, 0, 0, 0]  # invalid points count nothing
    assert (alone["tri_id"] == NO_TRI).all() and np.isposinf(alone["t"]).all() and (bits(alone["u"]) == 0).all()


# ---- 9. batch edges --------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 15, 16, 17, 33])
def test_batch_edges_write_nothing_past_n(ctx, n):
    import torch
    c = case(ctx, "suzanne")
    dev = torch.device("cuda", ctx.device)
    packed = np.zeros((n, 4), F)
    packed[:, 0:3], packed[:, 3] = c.pts[:n], np.inf
    p_dev = torch.from_numpy(packed).to(dev)
    exp = {key: val[:n] for key, val in c.exp.items()}
    for k in (3, 16):
        hits = torch.full((n * k + 64, 4), -7.5, dtype=torch.float32, device=dev)
        counts = torch.full((n + 64,), -3, dtype=torch.int32, device=dev)
        torch.cuda.synchronize()
        assert c.scene.closestPointsMultiDevice(p_dev.data_ptr(), n, k, hits.data_ptr(), counts.data_ptr()) == 0
        ctx.sync()
        h, cn = hits.cpu().numpy(), counts.cpu().numpy()
        assert np.all(h[n * k:] == F(-7.5)) and np.all(cn[n:] == -3)
        h = h[:n * k].reshape(n, k, 4)
        got = {"t": h[..., 0], "u": h[..., 1], "v": h[..., 2], "tri_id": h.view(np.uint32)[..., 3],
               "count": cn[:n].view(np.uint32)}
        assert_multi(got, exp, k, what=f"n = {n}")


def test_small_grid_strides_over_the_batches(ctx):
    c = case(ctx, "suzanne")
    small = beam.Context(device=0, params={"trace_grid": 2})  # 8 waves: about 30 batches each
    scene, keep = build(small, c.meshes)
    both(scene, c.pts, c.exp, (4, 16), what="two workgroups")
    scene.destroy()
    small.close()


# ---- 10. the stack's overflow area -----------------------------------------------------------------------
@pytest.mark.parametrize("k", [1, 4, 16])
def test_deep_chain_uses_the_overflow_area(k):
    """tests/deep_scenes.py's chain. With rmax = inf nothing is pruned before the first leaf, so a point beyond
    the origin corner, for which the chain's box is the nearest at every record, holds the siblings of the whole
    descent on its stack."""
    _, dup, leaf = ds.scene_of("deep")
    dctx = beam.Context(device=0, leaf_size=leaf)
    meshes = ds.deep_meshes(dup)
    verts = tri_vertices(meshes)
    rng = np.random.default_rng(9)
    pts = F(np.concatenate([-rng.uniform(2500, 6000, (40, 3)), [[-3000, -3000, -3000], [-1, -2, -3]],
                            rng.uniform(-2500, 3500, (30, 3))]))
    exp = brute_points_multi(pts, np.inf, verts, KMAX)
    scene, keep = build(dctx, meshes)
    for count_all in (False, True):
        res = scene.closestPointsMulti(pts, k=k, count_all=count_all, counters=True)
        deepest = int(res["counters"][3])
        print(f"deep chain, k = {k}, count_all = {count_all}: deepest stack {deepest} entries (LDS holds {QUAD_LDS})")
        assert deepest >= QUAD_LDS + 1, f"the overflow path did not run: deepest stack {deepest}"
        assert deepest <= ds.MAX_STACK
        assert_multi(res, exp, k, count_all, "deep chain, counting kernel")
        assert_multi(scene.closestPointsMulti(pts, k=k, count_all=count_all), exp, k, count_all, "deep chain")
    scene.destroy()
    dctx.close()


# ---- 11. other scene states --------------------------------------------------------------------------------
def test_query_after_refit(ctx):
    from test_gpu_points import make_points
    c = case(ctx, "suzanne")
    scene = beam.IScene.create(ctx)
    meshes = beam.upload_meshes(ctx, scene, c.meshes)
    scene.updateGPUScene()
    moved = []
    for m in c.meshes:  # scaled and sheared
        p = np.asarray(m["pos"], F).reshape(-1, 3)
        q = p.copy()
        q[:, 0] = p[:, 0] * F(1.25) + p[:, 1] * F(0.5)
        q[:, 1] = p[:, 1] * F(0.75)
        q[:, 2] = p[:, 2] * F(1.5) + p[:, 0] * F(0.25)
        moved.append(dict(m, pos=q))
    for m, mv in zip(meshes, moved):
        assert m.setVertexData(mv["pos"], mv["pos"].shape[0], 3, POS) == 0
    scene.refitGPUScene()
    pts = make_points(moved, 300, 21)
    exp = brute_points_multi(pts, np.inf, tri_vertices(moved), KMAX)
    both(scene, pts, exp, (4, 16), what="after refit")
    scene.destroy()


def test_instanced_scene(ctx):
    from test_gpu_points import make_points
    from test_instances_abi import MIRROR, rotation, xform_mesh
    c = case(ctx, "suzanne")
    base = c.meshes[0]
    x_rot = rotation((1, 2, 3), 0.7, (3.5, -0.25, 2.0))
    x_mir = np.array(MIRROR, F)
    x_mir[:, 3] = F([-3.25, 0.5, -1.0])
    scene = beam.IScene.create(ctx)
    mesh = beam.upload_meshes(ctx, scene, [base])[0]  # entry 0: the plain one
    assert scene.addInstance(mesh, x_rot) == 1
    assert scene.addInstance(mesh, x_mir) == 2
    scene.updateGPUScene()
    pre = [base, xform_mesh(x_rot, base), xform_mesh(x_mir, base)]  # the header's transform arithmetic, restated
    pts = make_points(pre, 300, 33)
    exp = brute_points_multi(pts, np.inf, tri_vertices(pre), KMAX)
    assert set((exp["tri_id"][:, 0] // c.verts.shape[0]).tolist()) == {0, 1, 2}
    both(scene, pts, exp, (4, 16), what="instances")
    scene.destroy()


def test_repeated_device_context_queries_on_the_root(ctx):
    c = case(ctx, "suzanne3")
    multi = beam.Context(devices=[0, 0])
    scene, keep = build(multi, c.meshes)
    both(scene, c.pts, c.exp, (5, 16), what="devices=[0, 0]")
    scene.destroy()
    multi.close()


# ---- 12. chaining on the device ----------------------------------------------------------------------------
def test_torch_chain_into_hit_attributes(ctx):
    """Points -> closestPointsMulti(k = 4) -> hitAttributes(position) on one stream without a wait or a host copy.
    The interpolated position of record (i, j) lies at distance t from point i within tests/test_gpu_points.py's
    bound for the same chain: 64 units of 2^-24 * (max |p_i| + max |vertex coordinate|), the unit computed from
    the inputs (the triangle function and the attribute path are the same as there)."""
    import torch
    from test_gpu_attrs import expected
    c = case(ctx, "suzanne")
    dev = torch.device("cuda", 0)
    tctx = beam.Context(device=0, stream=torch.cuda.current_stream(dev).cuda_stream)
    scene, keep = build(tctx, c.meshes)
    n, k = c.pts.shape[0], 4
    pts = torch.from_numpy(c.pts).to(dev)
    # no synchronisation from here to the end of the chain
    res = scene.closestPointsMulti(pts, k=k)
    assert res["hits"].is_cuda and res["hits"].shape == (n, k, 4) and res["tri_id"].dtype == torch.int32
    assert res["t"].shape == (n, k) and res["count"].shape == (n,) and res["count"].dtype == torch.int32
    (pos,) = scene.hitAttributes(res["hits"].view(-1, 4), [(POS, 3)])
    assert pos.is_cuda and pos.shape == (n * k, 3)
    gap = torch.linalg.vector_norm(pos.double().view(n, k, 3) - pts.double()[:, None, :], dim=2)
    m = 256  # a second query fed from the first one's result on the device: rmax = the fourth distance
    packed = torch.cat([pts[:m], res["t"][:m, 3:4].clamp_min(1e-30)], dim=1).contiguous()
    bounded = scene.closestPointsMulti(packed, k=k, count_all=True)
    torch.cuda.synchronize()
    hits = res["hits"].cpu().numpy()
    got = {"t": hits[..., 0], "u": hits[..., 1], "v": hits[..., 2], "tri_id": hits.view(np.uint32)[..., 3],
           "count": res["count"].cpu().numpy().view(np.uint32)}
    assert_multi(got, c.exp, k, what="torch path")
    flat = hits.reshape(-1, 4)
    want = expected(c.meshes, flat, POS, 3)
    assert np.array_equal(pos.cpu().numpy().view(np.uint32), want.view(np.uint32))
    scale = float(np.abs(c.pts).max() + np.abs(c.verts).max())
    worst = float(np.abs(gap.cpu().numpy() - c.exp["t"][:, :k].astype(np.float64)).max())
    print(f"chain: largest | |position - p| - t | = {worst / (2.0 ** -24 * scale):.2f} x 2^-24 x scale ({scale:.3g})")
    assert worst <= YARDSTICK_TOL_NO_SLIVERS * 2.0 ** -24 * scale
    assert YARDSTICK_TOL_NO_SLIVERS == 64.0
    rmax = np.maximum(c.exp["t"][:m, 3], F(1e-30))  # sqrtf(dd)^2 may round below dd: the brute force decides
    hb = bounded["hits"].cpu().numpy()
    gotb = {"t": hb[..., 0], "u": hb[..., 1], "v": hb[..., 2], "tri_id": hb.view(np.uint32)[..., 3],
            "count": bounded["count"].cpu().numpy().view(np.uint32)}
    assert_multi(gotb, brute_points_multi(c.pts[:m], rmax, c.verts, k), k, True, "torch path, rmax from the device")
    scene.destroy()
    tctx.close()


# ---- 13. errors ----------------------------------------------------------------------------------------------
def test_errors(ctx):
    import torch
    c = case(ctx, "suzanne")
    dev = torch.device("cuda", ctx.device)
    n = 64
    pts = torch.zeros((n + 1, 4), dtype=torch.float32, device=dev)
    out = torch.zeros((n * 16 + 1, 4), dtype=torch.float32, device=dev)
    cnt = torch.zeros((n + 1,), dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    pp, op, cp = pts.data_ptr(), out.data_ptr(), cnt.data_ptr()
    unbuilt = beam.IScene.create(ctx)
    assert unbuilt.closestPointsMultiDevice(pp, n, 4, op, cp) == _lib.ERROR_NOT_BUILT
    unbuilt.destroy()
    s = c.scene
    assert s.closestPointsMultiDevice(pp, n, 4, op) == 0 and s.closestPointsMultiDevice(pp, n, 16, op, cp, ALL) == 0
    assert s.closestPointsMultiDevice(pp, n, 0, 0, cp, ALL) == 0          # a pure count needs no hit records
    assert s.closestPointsMultiDevice(0, 0, 4, 0) == 0                    # n = 0: nothing to read or write
    assert s.closestPointsMultiDevice(pp, n, 0, op, cp) == BAD            # k = 0 without the flag
    assert s.closestPointsMultiDevice(pp, n, 17, op, cp) == BAD
    assert s.closestPointsMultiDevice(pp, n, 17, op, cp, ALL) == BAD
    for flags in (2, 3, 0x80000000):
        assert s.closestPointsMultiDevice(pp, n, 4, op, cp, flags) == BAD
    assert s.closestPointsMultiDevice(0, n, 4, op, cp) == BAD and s.closestPointsMultiDevice(pp, n, 4, 0, cp) == BAD
    assert s.closestPointsMultiDevice(pp, n, 4, op, 0, ALL) == BAD        # null counts with the flag
    off_p, off_o = pts.view(-1)[1:].data_ptr(), out.view(-1)[1:].data_ptr()  # 4 bytes in
    off_c = cnt.view(torch.int8)[1:].data_ptr()                              # 1 byte in
    assert off_p == pp + 4 and off_o == op + 4 and off_c == cp + 1
    assert s.closestPointsMultiDevice(off_p, n, 4, op, cp) == BAD
    assert s.closestPointsMultiDevice(pp, n, 4, off_o, cp) == BAD
    assert s.closestPointsMultiDevice(pp, n, 4, op, off_c) == BAD
    assert s.closestPointsMultiDevice(pp, n, 4, op, cnt[1:].data_ptr()) == 0  # counts are 4-byte aligned
    counters = np.zeros(4, np.uint64)
    assert s.closestPointsMultiDevice(pp, n, 17, op, cp, 0, counters) == BAD
    assert s.ctx.lib.bm_scene_closest_points_multi_counters(s.h, pp, n, 4, 0, op, cp, None) == BAD
    assert s.ctx.lib.bm_scene_closest_points_multi(None, pp, n, 4, 0, op, cp) == BAD  # a null handle
    ctx.sync()
    tiny = [{"pos": F([[0, 0, 1], [1, 0, 1], [0, 1, 1]]), "nrm": F([[0, 0, 1]] * 3), "idx": np.uint32([0, 1, 2])}]
    # (a BVH8 context exists in A/B builds only: the product library refuses to create one)
    for kw in ({"reference_kd": True}, {"reference_hash": True}, {"bvh_width": 2}):
        other = beam.Context(device=0, **kw)
        sc, keep = build(other, tiny)
        assert sc.closestPointsMultiDevice(pp, n, 4, op, cp) == BAD, kw
        assert sc.closestPointsMultiDevice(pp, n, 4, op, cp, ALL) == BAD, kw
        assert sc.closestPointsMultiDevice(pp, n, 4, op, cp, 0, counters) == BAD, kw
        sc.destroy()
        other.close()
