"""GPU checks of triangle overlap queries (bm_scene_overlap_triangles): the scene triangles that intersect each
triangle of a batch.

Every comparison is exact against brute_tris of tests/test_tris_abi.py: the header's triangle/triangle function
restated in numpy float32 and evaluated for every scene triangle and every query. The traversal prunes, the brute
force does not. LIST segments are compared as sorted sets with their counts. A reference is computed once per
scene and query set and left unchanged. No expected value comes from the library.
"""
from types import SimpleNamespace

import numpy as np
import pytest

import deep_scenes as ds
from raytracercuda_amd import _lib, beam, scenes
from test_boxes_abi import SHIFTS, sliver_meshes, translated, tri_vertices
from test_tris_abi import (F, INVALID, NO_TRI, RULES, brute_tris, moved, rule_scene, sliver_queries, suzanne_queries,
                           tri_tri)

pytestmark = pytest.mark.gpu

COUNT, ANY, LIST, SKIP = _lib.TRIS_COUNT, _lib.TRIS_ANY, _lib.TRIS_LIST, _lib.TRIS_PAD_SKIP_TRI
BAD = _lib.ERROR_INVALID_PARAMETER
QUAD_LDS = 24  # stack entries a query keeps in LDS (bm_trace_quad.h); beyond: the global overflow area
SENT = -7      # what the tests fill outputs with


def soup(verts):
    """One mesh of the triangles verts (ntri,3,3), unindexed."""
    v = np.ascontiguousarray(verts, F).reshape(-1, 3)
    return [{"pos": v, "nrm": np.tile(F([0, 0, 1]), (v.shape[0], 1)), "idx": np.arange(v.shape[0], dtype=np.uint32)}]


def build(ctx, meshes):
    scene = beam.IScene.create(ctx)
    keep = beam.upload_meshes(ctx, scene, meshes)
    scene.updateGPUScene()
    return scene, keep


def segments(res):
    return [np.sort(res["ids"][a:b]) for a, b in zip(res["offsets"][:-1], res["offsets"][1:])]


def assert_tris(scene, queries, exp, what="", modes=("count", "any", "list"), skip=None):
    """All of scene.overlapTriangles' modes over the queries equal brute_tris' answer exp."""
    n = queries.shape[0]
    if "count" in modes:
        res = scene.overlapTriangles(queries, mode="count", skip_tri=skip)
        bad = np.flatnonzero(res["count"] != exp["count"])
        assert bad.size == 0, f"{what}: count differs on {bad.size} of {n} queries, first {bad[:5]}"
    if "any" in modes:
        res = scene.overlapTriangles(queries, mode="any", skip_tri=skip)
        assert res["any"].dtype == bool and np.array_equal(res["any"], exp["count"] > 0), (what, "any")
    if "list" in modes:
        res = scene.overlapTriangles(queries, mode="list", skip_tri=skip)
        assert np.array_equal(res["count"], exp["count"]), (what, "list count")
        assert res["offsets"].shape == (n + 1,) and res["offsets"][0] == 0
        assert np.array_equal(np.diff(res["offsets"].astype(np.int64)), exp["count"]), (what, "offsets")
        assert res["ids"].shape == (int(exp["count"].sum()),)
        for i, (got, want) in enumerate(zip(segments(res), exp["ids"])):
            assert np.array_equal(got, want), (what, "ids of query", i)


def pack(queries, pad0=0xDEADBEEF):
    """bm_tri records (n, 12) float32; pad1 and pad2 hold junk, which is always ignored."""
    b = np.zeros((queries.shape[0], 12), F)
    b.reshape(-1, 3, 4)[:, :, 0:3] = queries
    u = b.view(np.uint32)
    u[:, 3], u[:, 7], u[:, 11] = pad0, 0x7FC00000, 0xFFFFFFFF
    return b


_CASE = {}


def case(ctx):
    """Suzanne as a GPU scene, the designed query set (every 16th triangle of the second Suzanne) and brute_tris'
    answer — made once per module run."""
    if not _CASE:
        meshes = scenes.load_mesh("suzanne")
        verts, queries = suzanne_queries()
        exp = brute_tris(queries, verts)
        exp["count"].setflags(write=False)
        queries.setflags(write=False)
        scene, keep = build(ctx, meshes)
        _CASE["c"] = SimpleNamespace(meshes=meshes, verts=verts, queries=queries, exp=exp, scene=scene, keep=keep)
    return _CASE["c"]


def teardown_module(module):
    for k in _CASE.values():
        k.scene.destroy()
    _CASE.clear()


# ---- 1. the rules ------------------------------------------------------------------------------------------
def test_rule_cases(ctx):
    verts, queries = rule_scene()
    exp = brute_tris(queries, verts)
    scene, keep = build(ctx, soup(verts))
    assert_tris(scene, queries, exp, "rules")
    res = scene.overlapTriangles(queries, mode="list")
    for i, (r, got) in enumerate(zip(RULES, segments(res))):
        assert (i in got.tolist()) == r[3], r[0]
    assert (res["count"][len(RULES):] == 0).all()  # the invalid queries
    scene.destroy()


# ---- 2. tiny scenes: the empty tree, the one-leaf root, a full leaf, a leaf plus one, several records ----------
@pytest.mark.parametrize("ntri", [0, 1, 2, 4, 5, 17])
def test_tiny_scenes(ctx, ntri):
    rng = np.random.default_rng(400 + ntri)
    verts = F(rng.uniform(-1, 1, (ntri, 1, 3)) + rng.uniform(-0.4, 0.4, (ntri, 3, 3)))
    scene, keep = build(ctx, soup(verts) if ntri else [])
    rand = F(rng.uniform(-1, 1, (180, 1, 3)) + rng.uniform(-0.6, 0.6, (180, 3, 3)))
    queries = np.concatenate([rand, verts, moved(verts)])  # the scene's own triangles, and slightly turned
    exp = brute_tris(queries, verts)
    hit = int((exp["count"] > 0).sum())
    assert (ntri == 0 and hit == 0) or (ntri <= hit < queries.shape[0])
    assert_tris(scene, queries, exp, f"{ntri} triangles")
    res = scene.overlapTriangles(queries, mode="count", counters=True)
    assert int(res["counters"][2]) == int(exp["count"].sum())
    if ntri == 0:  # a built scene with no triangles: zeros, nothing fetched or tested
        assert [int(x) for x in res["counters"]] == [0, 0, 0, 0] and (res["count"] == 0).all()
    scene.destroy()


# ---- 3. meshes ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["count", "any", "list"])
def test_suzanne(ctx, mode):
    c = case(ctx)
    cnt = c.exp["count"].astype(np.int64)
    assert c.queries.shape[0] == 968 and np.mean(cnt == 0) >= 0.25 and np.mean(cnt > 0) >= 0.25
    assert_tris(c.scene, c.queries, c.exp, "suzanne", modes=(mode,))


def test_any_equals_count_above_zero_and_stops_early(ctx):
    c = case(ctx)
    cnt = c.scene.overlapTriangles(c.queries, mode="count", counters=True)
    hit = c.scene.overlapTriangles(c.queries, mode="any", counters=True)
    assert np.array_equal(hit["any"], cnt["count"] > 0) and np.array_equal(cnt["count"], c.exp["count"])
    assert int(hit["counters"][2]) == int((cnt["count"] > 0).sum()) and int(cnt["counters"][2]) == int(cnt["count"].sum())
    n = c.queries.shape[0]
    print("suzanne, per query: " + ", ".join(f"{name} {int(r['counters'][0]) / n:.1f} node records, "
                                             f"{int(r['counters'][1]) / n:.1f} triangle tests"
                                             for name, r in (("count", cnt), ("any", hit))))
    assert int(hit["counters"][0]) <= int(cnt["counters"][0]) and int(hit["counters"][1]) < int(cnt["counters"][1])


# ---- 4. large coordinates and reconstructed vertices ---------------------------------------------------------
@pytest.mark.parametrize("shift", SHIFTS)
def test_translated_suzanne(ctx, shift):
    verts, queries = suzanne_queries(shift, every=32)
    exp = brute_tris(queries, verts)
    assert 0 < int((exp["count"] > 0).sum()) < queries.shape[0]
    scene, keep = build(ctx, translated(scenes.load_mesh("suzanne"), shift))
    assert_tris(scene, queries, exp, f"suzanne + {shift}")
    scene.destroy()


def test_slivers_across_magnitudes(ctx):
    meshes = sliver_meshes()
    verts = tri_vertices(meshes)
    queries = sliver_queries(verts)
    exp = brute_tris(queries, verts)
    assert 0 < int((exp["count"] > 0).sum()) < queries.shape[0]
    scene, keep = build(ctx, meshes)
    assert_tris(scene, queries, exp, "slivers")
    scene.destroy()


# ---- 5. LIST segmentation: exact, one short, a fixed stride ------------------------------------------------
def raw_list(scene, ctx, tris_dev, n, offsets, tail=64, flags=0):
    """One raw LIST call with sentinel-filled ids and counts; returns (ids with the tail, counts with the tail)."""
    import torch
    dev = tris_dev.device
    off = torch.from_numpy(np.ascontiguousarray(offsets, np.int32)).to(dev)
    ids = torch.full((int(offsets[-1]) + tail,), SENT, dtype=torch.int32, device=dev)
    out = torch.full((n + tail,), SENT, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    assert scene.overlapTrianglesDevice(tris_dev.data_ptr(), n, LIST, out.data_ptr(), off.data_ptr(), ids.data_ptr(),
                                        flags=flags) == 0
    ctx.sync()
    return ids.cpu().numpy(), out.cpu().numpy()


def test_list_segments_exact_short_and_strided(ctx):
    import torch
    c = case(ctx)
    exp = c.exp
    n = c.queries.shape[0]
    cnt = exp["count"].astype(np.int64)
    tris = torch.from_numpy(pack(c.queries)).to(torch.device("cuda", ctx.device))
    exact = np.concatenate([[0], np.cumsum(cnt)])
    short = np.concatenate([[0], np.cumsum(np.maximum(cnt - 1, 0))])
    stride = np.arange(n + 1) * 3
    full_ids, full_out = raw_list(c.scene, ctx, tris, n, exact)
    for name, off in (("exact", exact), ("one short", short), ("stride 3", stride)):
        ids, out = raw_list(c.scene, ctx, tris, n, off)
        assert np.array_equal(out[:n].view(np.uint32), exp["count"]), name  # the true count, whatever fitted
        assert (out[n:] == SENT).all() and (ids[off[-1]:] == SENT).all(), name  # nothing past the ends
        for i in range(n):
            seg = ids[off[i]:off[i + 1]]
            k = min(int(cnt[i]), seg.size)
            # the first k ids of the traversal's order (the exact run's segment), then an untouched tail
            assert np.array_equal(seg[:k], full_ids[exact[i]:exact[i] + k]), (name, i)
            assert (seg[k:] == SENT).all(), (name, i)
    for i in range(n):  # and the exact run holds each query's set
        assert np.array_equal(np.sort(full_ids[exact[i]:exact[i + 1]]).view(np.uint32), exp["ids"][i]), i
    assert (short[1:] - short[:-1] < cnt).sum() == int((cnt > 0).sum()) and (cnt > 3).any() and (cnt < 3).any()
    # a null out_dev: the ids alone
    dev = tris.device
    ids2 = torch.full((int(exact[-1]) + 64,), SENT, dtype=torch.int32, device=dev)
    off = torch.from_numpy(exact.astype(np.int32)).to(dev)
    torch.cuda.synchronize()
    assert c.scene.overlapTrianglesDevice(tris.data_ptr(), n, LIST, 0, off.data_ptr(), ids2.data_ptr()) == 0
    ctx.sync()
    assert np.array_equal(ids2.cpu().numpy(), full_ids)


def test_list_order_is_the_same_on_every_call_and_grid(ctx):
    c = case(ctx)
    first = c.scene.overlapTriangles(c.queries, mode="list")
    again = c.scene.overlapTriangles(c.queries, mode="list")
    assert np.array_equal(first["ids"], again["ids"]) and np.array_equal(first["offsets"], again["offsets"])
    small = beam.Context(device=0, params={"trace_grid": 2})  # 8 waves stride over the 61 batches
    scene, keep = build(small, c.meshes)
    other = scene.overlapTriangles(c.queries, mode="list")
    assert np.array_equal(first["ids"], other["ids"]) and np.array_equal(first["offsets"], other["offsets"])
    assert_tris(scene, c.queries, c.exp, "two workgroups", modes=("count", "any"))
    scene.destroy()
    small.close()


# ---- 6. the skip filter ------------------------------------------------------------------------------------
def test_pad_skip_tri(ctx):
    import torch
    c = case(ctx)
    n = c.queries.shape[0]
    cnt = c.exp["count"].astype(np.int64)
    # name, per query, the first id of its set (a query that hits nothing: an id it does not hit)
    skip = np.array([int(a[0]) if a.size else 5 for a in c.exp["ids"]], np.uint32)
    exp = brute_tris(c.queries, c.verts, skip=skip)
    assert np.array_equal(exp["count"].astype(np.int64), cnt - (cnt > 0))  # exactly the named id goes
    for i in range(n):
        assert exp["ids"][i].tolist() == c.exp["ids"][i].tolist()[1:], i
    assert_tris(c.scene, c.queries, exp, "skip the first id", skip=skip)
    # NO_TRI and ids past the scene skip nothing
    ntri = c.verts.shape[0]
    nothing = np.where(np.arange(n) % 3 == 0, NO_TRI, np.where(np.arange(n) % 3 == 1, ntri, ntri + 12345)).astype(np.uint32)
    assert_tris(c.scene, c.queries, c.exp, "ids that name no triangle", skip=nothing)
    # without the flag pad0 is ignored: the same ids in pad0, flags = 0
    dev = torch.device("cuda", ctx.device)
    tris = torch.from_numpy(pack(c.queries, pad0=skip)).to(dev)
    out = torch.full((n,), SENT, dtype=torch.int32, device=dev)
    flagged = torch.full((n,), SENT, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    assert c.scene.overlapTrianglesDevice(tris.data_ptr(), n, COUNT, out.data_ptr(), flags=0) == 0
    assert c.scene.overlapTrianglesDevice(tris.data_ptr(), n, COUNT, flagged.data_ptr(), flags=SKIP) == 0
    ctx.sync()
    assert np.array_equal(out.cpu().numpy().view(np.uint32), c.exp["count"])
    assert np.array_equal(flagged.cpu().numpy().view(np.uint32), exp["count"])
    # and packed records with their own pad0 through the Python layer
    res = c.scene.overlapTriangles(pack(c.queries, pad0=skip), mode="count", skip_tri=True)
    assert np.array_equal(res["count"], exp["count"])


# ---- 7. invalid queries ------------------------------------------------------------------------------------
def test_invalid_queries_find_nothing(ctx):
    c = case(ctx)
    queries = c.queries.copy()
    n = queries.shape[0]
    sel = np.arange(3, n, 7)
    bad = F(INVALID)
    queries[sel] = bad[(sel // 7) % bad.shape[0]]
    invalid = np.zeros(n, bool)
    invalid[sel] = True
    exp = brute_tris(queries, c.verts)
    assert (exp["count"][invalid] == 0).all() and np.array_equal(exp["count"][~invalid], c.exp["count"][~invalid])
    assert (exp["count"][~invalid] > 0).any()
    assert_tris(c.scene, queries, exp, "invalid queries")
    for mode in ("count", "any", "list"):
        alone = c.scene.overlapTriangles(queries[invalid], mode=mode, counters=True)
        assert [int(x) for x in alone["counters"]] == [0, 0, 0, 0], mode  # invalid queries count nothing
        assert not alone["any" if mode == "any" else "count"].any()


# ---- 8. batch edges ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 15, 16, 17, 33])
def test_batch_edges_write_nothing_past_n(ctx, n):
    import torch
    c = case(ctx)
    first = int(np.flatnonzero(c.exp["count"] > 0)[0])  # a window with hits in it
    at = max(0, min(first - n // 2, c.queries.shape[0] - n))
    queries, cnt = c.queries[at:at + n], c.exp["count"][at:at + n]
    assert cnt.any()
    dev = torch.device("cuda", ctx.device)
    tris = torch.from_numpy(pack(queries)).to(dev)
    out = torch.full((n + 64,), SENT, dtype=torch.int32, device=dev)
    flag = torch.full((n + 64,), SENT, dtype=torch.int8, device=dev)
    torch.cuda.synchronize()
    assert c.scene.overlapTrianglesDevice(tris.data_ptr(), n, COUNT, out.data_ptr()) == 0
    assert c.scene.overlapTrianglesDevice(tris.data_ptr(), n, ANY, flag.data_ptr()) == 0
    ctx.sync()
    o, f = out.cpu().numpy(), flag.cpu().numpy()
    assert np.array_equal(o[:n].view(np.uint32), cnt) and (o[n:] == SENT).all()
    assert np.array_equal(f[:n], (cnt > 0).astype(np.int8)) and (f[n:] == SENT).all()
    off = np.concatenate([[0], np.cumsum(cnt.astype(np.int64))])
    ids, lout = raw_list(c.scene, ctx, tris, n, off)
    assert np.array_equal(lout[:n].view(np.uint32), cnt) and (lout[n:] == SENT).all() and (ids[off[-1]:] == SENT).all()
    for i in range(n):
        assert np.array_equal(np.sort(ids[off[i]:off[i + 1]]).view(np.uint32), c.exp["ids"][at + i]), i


# ---- 9. the stack's overflow area --------------------------------------------------------------------------
def test_deep_chain_uses_the_overflow_area():
    """tests/deep_scenes.py's chain under a query triangle whose bounds hold it: nothing is pruned, so the siblings
    of the whole descent wait on the stack."""
    _, dup, leaf = ds.scene_of("deep")
    dctx = beam.Context(device=0, leaf_size=leaf)
    meshes = ds.deep_meshes(dup)
    verts = tri_vertices(meshes)
    p = verts.reshape(-1, 3)
    lo, hi = p.min(axis=0), p.max(axis=0)
    span = np.stack([lo - F(1), hi + F(1), (lo + hi) * F(0.5)])[None]  # the scene's diagonal
    queries = np.concatenate([span, verts[::max(1, verts.shape[0] // 40)], moved(verts[::max(1, verts.shape[0] // 30)])])
    queries = np.ascontiguousarray(queries, F)
    exp = brute_tris(queries, verts)
    assert (exp["count"][1:] > 0).any()
    scene, keep = build(dctx, meshes)
    for mode in ("count", "list"):
        res = scene.overlapTriangles(queries, mode=mode, counters=True)
        deepest = int(res["counters"][3])
        print(f"deep chain, {mode}: deepest stack {deepest} entries (LDS holds {QUAD_LDS})")
        assert deepest >= QUAD_LDS + 1, f"the overflow path did not run: deepest stack {deepest}"
        assert deepest <= ds.MAX_STACK
        assert np.array_equal(res["count"], exp["count"])
    one = scene.overlapTriangles(queries[:1], mode="count", counters=True)
    assert int(one["counters"][1]) == verts.shape[0]  # the spanning query reaches every leaf once
    assert_tris(scene, queries, exp, "deep chain")
    scene.destroy()
    dctx.close()


# ---- 10. other scene states --------------------------------------------------------------------------------
def test_query_after_refit(ctx):
    c = case(ctx)
    scene = beam.IScene.create(ctx)
    meshes = beam.upload_meshes(ctx, scene, c.meshes)
    scene.updateGPUScene()
    changed = []
    for m in c.meshes:  # scaled and sheared
        p = np.asarray(m["pos"], F).reshape(-1, 3)
        q = p.copy()
        q[:, 0] = p[:, 0] * F(1.25) + p[:, 1] * F(0.5)
        q[:, 1] = p[:, 1] * F(0.75)
        q[:, 2] = p[:, 2] * F(1.5) + p[:, 0] * F(0.25)
        changed.append(dict(m, pos=q))
    for m, mv in zip(meshes, changed):
        assert m.setVertexData(mv["pos"], mv["pos"].shape[0], 3, beam.VERTEX_DATA_POSITION) == 0
    scene.refitGPUScene()
    verts = tri_vertices(changed)
    queries = np.concatenate([moved(verts[::32]), c.queries[::4]])  # about the new shape, and about the old one
    exp = brute_tris(queries, verts)
    assert 0 < int((exp["count"] > 0).sum()) < queries.shape[0]
    assert_tris(scene, queries, exp, "after refit")
    scene.destroy()


def test_instanced_scene(ctx):
    from test_instances_abi import MIRROR, rotation, xform_mesh
    c = case(ctx)
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
    verts = tri_vertices(pre)
    queries = np.ascontiguousarray(moved(verts[::48]))
    exp = brute_tris(queries, verts)
    n1 = c.verts.shape[0]
    assert {int(a[0]) // n1 for a in exp["ids"] if a.size} == {0, 1, 2}
    assert_tris(scene, queries, exp, "instances")
    scene.destroy()


# ---- 11. the Python layer ----------------------------------------------------------------------------------
def test_torch_chain_into_hit_attributes(ctx):
    """Triangles -> overlapTriangles(mode="list") -> the ids as bm_hit records -> hitAttributes(BM_ATTR_MESH_FACE)
    on one stream: which mesh and face each listed triangle is."""
    import torch
    c = case(ctx)
    dev = torch.device("cuda", 0)
    tctx = beam.Context(device=0, stream=torch.cuda.current_stream(dev).cuda_stream)
    meshes = c.meshes + translated(c.meshes, (0.004, 0.002, -0.003))  # two meshes: the owner is not always mesh 0
    verts = tri_vertices(meshes)
    scene, keep = build(tctx, meshes)
    exp = brute_tris(c.queries, verts)
    q = torch.from_numpy(c.queries.copy()).to(dev)
    res = scene.overlapTriangles(q, mode="list")
    assert res["ids"].is_cuda and res["ids"].dtype == torch.int32 and res["offsets"].shape == (q.shape[0] + 1,)
    hits = torch.zeros((res["ids"].shape[0], 4), dtype=torch.float32, device=dev)
    hits.view(torch.int32)[:, 3] = res["ids"]
    (face,) = scene.hitAttributes(hits, [(beam.ATTR_MESH_FACE, 2)])
    hit = scene.overlapTriangles(torch.from_numpy(pack(c.queries)).to(dev), mode="any")["any"]
    torch.cuda.synchronize()
    got = {k: v.cpu().numpy().view(np.uint32) for k, v in res.items()}
    assert np.array_equal(got["count"], exp["count"])
    for i, (seg, want) in enumerate(zip(segments(got), exp["ids"])):
        assert np.array_equal(seg, want), i
    n1 = c.verts.shape[0]
    ids = got["ids"].astype(np.int64)
    assert np.array_equal(face.cpu().numpy(), np.stack([ids // n1, ids % n1], axis=1))
    assert len(c.meshes) == 1 and set((ids // n1).tolist()) == {0, 1}
    assert np.array_equal(hit.cpu().numpy(), exp["count"] > 0)
    scene.destroy()
    tctx.close()


def closed_box(lo, hi):
    """A closed box of 8 vertices and 12 triangles."""
    lo, hi = np.asarray(lo, np.float64), np.asarray(hi, np.float64)
    pos = F([[(lo, hi)[(i >> k) & 1][k] for k in range(3)] for i in range(8)])
    quads = [(0, 2, 3, 1), (4, 5, 7, 6), (0, 1, 5, 4), (2, 6, 7, 3), (0, 4, 6, 2), (1, 3, 7, 5)]
    idx = np.uint32([t for a, b, cc, d in quads for t in ((a, b, cc), (a, cc, d))]).reshape(-1)
    return {"pos": pos, "nrm": np.tile(F([0, 0, 1]), (8, 1)), "idx": idx}


def brute_self(meshes):
    """selfIntersections' definition by brute force: the pairs i < j that tri_tri accepts in either direction, on
    the record's vertices, less the pairs of one mesh that share a vertex index."""
    from test_boxes_abi import record_vertices
    verts = tri_vertices(meshes)
    v = np.stack(record_vertices(verts), axis=1)
    n = v.shape[0]
    i, j = np.nonzero(np.triu(np.ones((n, n), bool), 1))
    acc = tri_tri(v[i, 0], v[i, 1], v[i, 2], v[j, 0], v[j, 1], v[j, 2]) | \
        tri_tri(v[j, 0], v[j, 1], v[j, 2], v[i, 0], v[i, 1], v[i, 2])
    owner = np.concatenate([np.full(len(m["idx"]) // 3, k) for k, m in enumerate(meshes)])
    vidx = np.concatenate([np.asarray(m["idx"], np.int64).reshape(-1, 3) for m in meshes])
    touch = (owner[i] == owner[j]) & (vidx[i][:, :, None] == vidx[j][:, None, :]).any(axis=(1, 2))
    keep = acc & ~touch
    return np.stack([i[keep], j[keep]], axis=1).astype(np.int64), owner


def test_self_intersections(ctx):
    two = [closed_box((0, 0, 0), (1, 1, 1)), closed_box((0.4, 0.3, 0.6), (1.3, 1.2, 1.7))]
    want, owner = brute_self(two)
    assert want.shape[0] > 0 and (owner[want[:, 0]] != owner[want[:, 1]]).all()  # only the cross-mesh pairs are left
    scene, keep = build(ctx, two)
    got = scene.selfIntersections(indices=[m["idx"] for m in two])
    assert got.dtype == np.int64 and np.array_equal(got, want)
    # every pair, neighbours included, with a shared() that leaves nothing out: more pairs, all of the former among them
    everything = scene.selfIntersections(shared=lambda i, j: False)
    assert everything.shape[0] > got.shape[0] and {tuple(r) for r in got.tolist()} <= {tuple(r) for r in everything.tolist()}
    with pytest.raises(beam.BeamError):
        scene.selfIntersections()
    scene.destroy()
    one = [closed_box((-1, -2, -3), (1.5, 0.5, 2))]
    want, _ = brute_self(one)
    assert want.shape == (0, 2)
    scene, keep = build(ctx, one)
    assert scene.selfIntersections(indices=[one[0]["idx"]]).shape == (0, 2)
    scene.destroy()


# ---- 12. errors ----------------------------------------------------------------------------------------------
def test_errors(ctx):
    import torch
    c = case(ctx)
    dev = torch.device("cuda", ctx.device)
    n = 64
    tris = torch.zeros((n + 1, 12), dtype=torch.float32, device=dev)
    out = torch.zeros((n + 2,), dtype=torch.int32, device=dev)
    off = torch.zeros((n + 2,), dtype=torch.int32, device=dev)
    ids = torch.zeros((64,), dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    tp, op, fp, ip = tris.data_ptr(), out.data_ptr(), off.data_ptr(), ids.data_ptr()
    unbuilt = beam.IScene.create(ctx)
    assert unbuilt.overlapTrianglesDevice(tp, n, COUNT, op) == _lib.ERROR_NOT_BUILT
    unbuilt.destroy()
    s = c.scene
    q = s.overlapTrianglesDevice
    assert q(tp, n, COUNT, op) == 0 and q(tp, n, ANY, op) == 0
    assert q(tp, n, LIST, op, fp, ip) == 0 and q(tp, n, LIST, 0, fp, ip) == 0
    assert q(tp, n, COUNT, op, flags=SKIP) == 0 and q(tp, n, LIST, op, fp, ip, flags=SKIP) == 0
    assert q(0, 0, COUNT, 0) == 0 and q(0, 0, LIST, 0) == 0  # n = 0: nothing read
    for mode in (3, 4, 0x80000000):
        assert q(tp, n, mode, op, fp, ip) == BAD
    for flags in (2, 3, 4, 0x80000000):
        assert q(tp, n, COUNT, op, flags=flags) == BAD
    assert q(0, n, COUNT, op) == BAD and q(tp, n, COUNT, 0) == BAD
    assert q(tp, n, ANY, 0) == BAD
    assert q(tp, n, LIST, op, 0, ip) == BAD and q(tp, n, LIST, op, fp, 0) == BAD
    off_b = tris.view(-1)[1:].data_ptr()            # 4 bytes in
    byte = lambda t: t.view(torch.int8)[1:].data_ptr()  # 1 byte in
    assert off_b == tp + 4 and byte(out) == op + 1
    assert q(off_b, n, COUNT, op) == BAD
    assert q(tris.view(-1)[4:].data_ptr(), n, COUNT, op) == 0  # records are 16-byte aligned
    assert q(tp, n, COUNT, byte(out)) == BAD
    assert q(tp, n, ANY, byte(out)) == 0                        # the byte plane: any address
    assert q(tp, n, LIST, byte(out), fp, ip) == BAD
    assert q(tp, n, LIST, op, byte(off), ip) == BAD
    assert q(tp, n, LIST, op, fp, byte(ids)) == BAD
    assert q(tp, n, LIST, out[1:].data_ptr(), off[1:].data_ptr(), ids[1:].data_ptr()) == 0
    assert q(tp, n, COUNT, op, byte(off), byte(ids)) == 0       # COUNT ignores offsets and ids
    counters = np.zeros(4, np.uint64)
    assert q(tp, n, 3, op, counters=counters) == BAD
    assert s.ctx.lib.bm_scene_overlap_triangles_counters(s.h, tp, n, COUNT, 0, op, None, None, None) == BAD
    assert s.ctx.lib.bm_scene_overlap_triangles(None, tp, n, COUNT, 0, op, None, None) == BAD  # a null handle
    ctx.sync()
    with pytest.raises(beam.BeamError):
        s.overlapTriangles(np.zeros((4, 3, 3), F), mode="all")
    tiny = [{"pos": F([[0, 0, 1], [1, 0, 1], [0, 1, 1]]), "nrm": F([[0, 0, 1]] * 3), "idx": np.uint32([0, 1, 2])}]
    # (a BVH8 context exists in A/B builds only: the product library refuses to create one)
    for kw in ({"reference_kd": True}, {"reference_hash": True}, {"bvh_width": 2}):
        other = beam.Context(device=0, **kw)
        sc, keep = build(other, tiny)
        for mode in (COUNT, ANY, LIST):
            assert sc.overlapTrianglesDevice(tp, n, mode, op, fp, ip) == BAD, kw
        assert sc.overlapTrianglesDevice(tp, n, COUNT, op, counters=counters) == BAD, kw
        sc.destroy()
        other.close()
