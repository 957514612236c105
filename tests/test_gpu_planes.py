"""GPU checks of plane section queries (bm_scene_section_planes): the triangles each plane of a batch crosses and
their cut segments.

Every comparison is exact against brute_planes of tests/plane_scenes.py: the header's rule restated in numpy
float32 on the meshes' own vertices and evaluated for every triangle and every plane. The traversal prunes, the
brute force does not. LIST ids are compared as sorted sets with their counts, segments as exact 32-byte records
keyed by triangle id. A reference is computed once per scene and plane set and left unchanged. No expected value
comes from the library.
"""
from types import SimpleNamespace

import numpy as np
import pytest

import deep_scenes as ds
import plane_scenes as ps
from plane_scenes import F, U, brute_planes, soup, tri_vertices
from raytracercuda_amd import _lib, beam, scenes

pytestmark = pytest.mark.gpu

COUNT, ANY, LIST = _lib.PLANES_COUNT, _lib.PLANES_ANY, _lib.PLANES_LIST
BAD = _lib.ERROR_INVALID_PARAMETER
QUAD_LDS = 24  # stack entries a query keeps in LDS (bm_trace_quad.h); beyond: the global overflow area
SENT = -7      # what the tests fill outputs with
SENT_U = np.array([SENT], np.int32).view(U)[0]


def build(ctx, meshes):
    scene = beam.IScene.create(ctx)
    keep = beam.upload_meshes(ctx, scene, meshes)
    scene.updateGPUScene()
    return scene, keep


def pack(pts, nrm):
    p = np.zeros((pts.shape[0], 8), F)
    p[:, 0:3], p[:, 4:7] = pts, nrm
    p.view(U)[:, 3], p.view(U)[:, 7] = 0xDEADBEEF, 0x7FC00000  # the pad words are ignored
    return p


def raw_list(scene, ctx, planes_dev, n, offsets, ids=True, segs=True, out=True, tail=64):
    """One raw LIST call with sentinel-filled outputs; returns (ids, segment records (k, 8) uint32, counts), each
    with its tail, None where the pointer was null."""
    import torch
    dev = planes_dev.device
    off = torch.from_numpy(np.ascontiguousarray(offsets, np.int32)).to(dev)
    total = int(offsets[-1])
    idt = torch.full((total + tail,), SENT, dtype=torch.int32, device=dev) if ids else None
    sgt = torch.full((total + tail, 8), SENT, dtype=torch.int32, device=dev) if segs else None
    ott = torch.full((n + tail,), SENT, dtype=torch.int32, device=dev) if out else None
    torch.cuda.synchronize()
    assert scene.sectionPlanesDevice(planes_dev.data_ptr(), n, LIST, ott.data_ptr() if out else 0, off.data_ptr(),
                                     idt.data_ptr() if ids else 0, sgt.data_ptr() if segs else 0) == 0
    ctx.sync()
    host = lambda t: None if t is None else t.cpu().numpy()
    s = host(sgt)
    return host(idt), None if s is None else s.view(U), host(ott)


def by_id(rec):
    return rec[np.argsort(rec[:, 3], kind="stable")]


def assert_planes(scene, ctx, pts, nrm, exp, what="", modes=("count", "any", "list", "segments", "raw")):
    """scene.sectionPlanes' modes, and the raw LIST call with ids only, segments only and both, equal exp."""
    import torch
    n = pts.shape[0]
    cnt = exp["count"].astype(np.int64)
    if "count" in modes:
        res = scene.sectionPlanes(pts, nrm, mode="count")
        bad = np.flatnonzero(res["count"] != exp["count"])
        assert bad.size == 0, f"{what}: count differs on {bad.size} of {n} planes, first {bad[:5]}"
    if "any" in modes:
        res = scene.sectionPlanes(pts, nrm, mode="any")
        assert res["any"].dtype == bool and np.array_equal(res["any"], exp["count"] > 0), (what, "any")
    if "list" in modes:
        res = scene.sectionPlanes(pts, nrm, mode="list")
        assert np.array_equal(res["count"], exp["count"]), (what, "list count")
        assert res["offsets"].shape == (n + 1,) and res["offsets"][0] == 0
        assert np.array_equal(np.diff(res["offsets"].astype(np.int64)), cnt), (what, "offsets")
        for i, want in enumerate(exp["ids"]):
            assert np.array_equal(np.sort(res["ids"][res["offsets"][i]:res["offsets"][i + 1]]), want), (what, "ids", i)
    if "segments" in modes:
        off, ids, a, b = scene.sectionPlanes(pts, nrm, mode="segments")
        assert np.array_equal(np.diff(off.astype(np.int64)), cnt) and ids.shape == (int(cnt.sum()),), (what, "segments")
        assert a.shape == (ids.shape[0], 3) and b.shape == a.shape and a.dtype == F
        for i, want in enumerate(exp["segs"]):
            sl = slice(int(off[i]), int(off[i + 1]))
            order = np.argsort(ids[sl], kind="stable")
            assert np.array_equal(ids[sl][order], want[:, 3]), (what, "segment ids", i)
            assert np.array_equal(a[sl][order].view(U), want[:, 0:3]), (what, "a of plane", i)
            assert np.array_equal(b[sl][order].view(U), want[:, 4:7]), (what, "b of plane", i)
    if "raw" in modes and n:
        planes = torch.from_numpy(pack(pts, nrm)).to(torch.device("cuda", ctx.device))
        off = np.concatenate([[0], np.cumsum(cnt)])
        both = raw_list(scene, ctx, planes, n, off)
        ids_only = raw_list(scene, ctx, planes, n, off, segs=False)
        segs_only = raw_list(scene, ctx, planes, n, off, ids=False, out=False)
        assert np.array_equal(both[0], ids_only[0]) and np.array_equal(both[1], segs_only[1]), (what, "ids / segs / both")
        assert np.array_equal(both[2], ids_only[2]) and np.array_equal(both[2][:n].view(U), exp["count"])
        ids, seg, out = both
        assert (ids[off[-1]:] == SENT).all() and (seg[off[-1]:] == SENT_U).all() and (out[n:] == SENT).all()
        assert np.array_equal(ids[:off[-1]].view(U), seg[:off[-1], 3])  # slot j of ids is slot j of segs
        for i, want in enumerate(exp["segs"]):
            assert np.array_equal(by_id(seg[off[i]:off[i + 1]]), want), (what, "segment records of plane", i)
            assert ps.loop_closure(want) == ps.loop_closure(seg[off[i]:off[i + 1]])


_CASES = {}


def case(ctx, name):
    """Meshes, GPU scene, planes and brute_planes' answer — made once per module run. torus, icosphere: the
    designed sets; suzanne: 64 planes of its designed set."""
    if name not in _CASES:
        if name == "torus":
            meshes, verts, pts, nrm, groups = ps.torus_case()
        elif name == "icosphere":
            meshes, verts, pts, nrm, groups = ps.icosphere_case()
        else:
            meshes = scenes.load_mesh(name)
            verts = tri_vertices(meshes)
            pts, nrm, groups = ps.designed_planes(verts, seed=5)
            extra = ps.designed_planes(verts, seed=6)
            pts, nrm = np.concatenate([pts, extra[0][:10]]), np.concatenate([nrm, extra[1][:10]])
        exp = brute_planes(pts, nrm, verts)
        for a in [exp["count"]] + exp["ids"] + exp["segs"]:
            a.setflags(write=False)
        scene, keep = build(ctx, meshes)
        _CASES[name] = SimpleNamespace(meshes=meshes, verts=verts, scene=scene, keep=keep, pts=pts, nrm=nrm,
                                       groups=groups, exp=exp)
    return _CASES[name]


def teardown_module(module):
    for k in _CASES.values():
        k.scene.destroy()
    _CASES.clear()


# ---- 1. the rules ----------------------------------------------------------------------------------------
def test_rule_cases(ctx):
    verts, pts, nrm = ps.rule_scene()
    pts, nrm = np.concatenate([pts, pts[:1]]), np.concatenate([nrm, -nrm[:1]])  # and the opposite normal
    exp = brute_planes(pts, nrm, verts)
    assert exp["ids"][0].tolist() == [i for i, r in enumerate(ps.RULES) if r[2]]
    assert exp["ids"][-1].tolist() == [0, 2, 7, 8, 10] and (exp["count"][1:-1] == 0).all()
    scene, keep = build(ctx, soup(verts))
    assert_planes(scene, ctx, pts, nrm, exp, "rules")
    off, ids, a, b = scene.sectionPlanes(pts, nrm, mode="segments")
    got = {int(i): (a[j], b[j]) for j, i in enumerate(ids[off[0]:off[1]])}
    v = F(ps.RULES[1][1])[0]  # touching from below in one vertex: a == b == that vertex's bits
    assert np.array_equal(got[1][0].view(U), v.view(U)) and np.array_equal(got[1][1].view(U), v.view(U))
    scene.destroy()


# ---- 2. tiny scenes: the empty tree, the one-leaf root, a full leaf, a leaf plus one, several records ------
@pytest.mark.parametrize("ntri", [0, 1, 2, 4, 5, 17])
def test_tiny_scenes(ctx, ntri):
    rng = np.random.default_rng(400 + ntri)
    verts = F(rng.uniform(-1, 1, (ntri, 1, 3)) + rng.uniform(-0.4, 0.4, (ntri, 3, 3)))
    scene, keep = build(ctx, soup(verts) if ntri else [])
    pts = F(rng.uniform(-1.2, 1.2, (203, 3)))
    nrm = F(rng.normal(size=(203, 3)))
    pts[:ntri] = verts[:, 0]  # through a vertex of each triangle
    exp = brute_planes(pts, nrm, verts)
    assert ntri == 0 or 0 < int((exp["count"] > 0).sum()) < 203
    assert_planes(scene, ctx, pts, nrm, exp, f"{ntri} triangles")
    res = scene.sectionPlanes(pts, nrm, mode="count", counters=True)
    assert int(res["counters"][2]) == int(exp["count"].sum())
    if ntri == 0:  # a built scene with no triangles: zeros, nothing fetched or tested
        assert [int(x) for x in res["counters"]] == [0, 0, 0, 0] and (res["count"] == 0).all()
    scene.destroy()


# ---- 3. the closed meshes: every designed plane, every mode, ids only, segments only and both --------------
@pytest.mark.parametrize("mode", ["count", "any", "list", "segments", "raw"])
@pytest.mark.parametrize("name", ["torus", "icosphere"])
def test_closed_meshes(ctx, name, mode):
    c = case(ctx, name)
    cnt = c.exp["count"]
    assert (cnt[c.groups["miss"]] == 0).all() and (cnt[c.groups["vertex"]] > 0).all() and (cnt[c.groups["rows"]] > 0).all()
    assert_planes(c.scene, ctx, c.pts, c.nrm, c.exp, name, modes=(mode,))


@pytest.mark.parametrize("name", ["torus", "icosphere"])
def test_loops_close_on_the_gpus_own_segments(ctx, name):
    """On a closed mesh the a and the b of each plane's segments are the same multiset of points, byte for byte;
    chainSegments links them into loops with nothing left open."""
    c = case(ctx, name)
    off, ids, a, b = c.scene.sectionPlanes(c.pts, c.nrm, mode="segments")
    for i in range(c.pts.shape[0]):
        sl = slice(int(off[i]), int(off[i + 1]))
        rec = np.zeros((sl.stop - sl.start, 8), U)
        rec[:, 0:3], rec[:, 4:7] = a[sl].view(U), b[sl].view(U)
        assert ps.loop_closure(rec), (name, i)
        lp, ch = beam.chainSegments(a[sl], b[sl])
        assert not ch and (len(lp) >= 1) == bool((rec[:, 0:3] != rec[:, 4:7]).any()), (name, i)
    if name == "torus":  # the plane of the vertex rows at z = 0: the two equators, 24 edges each
        r = c.groups["rows"].start
        lp, ch = beam.chainSegments(a[off[r]:off[r + 1]], b[off[r]:off[r + 1]])
        assert sorted(len(x) for x in lp) == [24, 24] and not ch and off[r + 1] - off[r] == 96


# ---- 4. meshes; large coordinates ------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["count", "any", "list", "raw"])
def test_suzanne(ctx, mode):
    c = case(ctx, "suzanne")
    assert c.pts.shape[0] == 64 and 0.5 < np.mean(c.exp["count"] > 0) < 1
    assert_planes(c.scene, ctx, c.pts, c.nrm, c.exp, "suzanne", modes=(mode,))


def test_translated_suzanne(ctx):
    moved = ps.translated(scenes.load_mesh("suzanne"), (65536, 0, 0))
    verts = tri_vertices(moved)
    pts, nrm, groups = ps.designed_planes(verts, seed=8)
    exp = brute_planes(pts, nrm, verts)
    assert (exp["count"][groups["vertex"]] > 0).all()
    scene, keep = build(ctx, moved)
    assert_planes(scene, ctx, pts, nrm, exp, "suzanne + (65536, 0, 0)", modes=("count", "any", "raw"))
    scene.destroy()


def test_slivers_whose_records_differ_from_their_vertices(ctx):
    """v0 + e1 of the build's record is not the mesh's v1 on these triangles: the query reads the mesh."""
    from test_boxes_abi import sliver_meshes
    meshes = sliver_meshes()
    verts = tri_vertices(meshes)
    pts, nrm, groups = ps.designed_planes(verts, seed=9)
    exp = brute_planes(pts, nrm, verts)
    assert exp["count"].max() > 40
    scene, keep = build(ctx, meshes)
    assert_planes(scene, ctx, pts, nrm, exp, "slivers", modes=("count", "any", "raw"))
    scene.destroy()


# ---- 5. batch edges --------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 15, 16, 17, 33])
def test_batch_edges_write_nothing_past_n(ctx, n):
    import torch
    c = case(ctx, "torus")
    dev = torch.device("cuda", ctx.device)
    planes = torch.from_numpy(pack(c.pts[:n], c.nrm[:n])).to(dev)
    cnt = c.exp["count"][:n]
    out = torch.full((n + 64,), SENT, dtype=torch.int32, device=dev)
    flag = torch.full((n + 64,), SENT, dtype=torch.int8, device=dev)
    torch.cuda.synchronize()
    assert c.scene.sectionPlanesDevice(planes.data_ptr(), n, COUNT, out.data_ptr()) == 0
    assert c.scene.sectionPlanesDevice(planes.data_ptr(), n, ANY, flag.data_ptr()) == 0
    ctx.sync()
    o, f = out.cpu().numpy(), flag.cpu().numpy()
    assert np.array_equal(o[:n].view(U), cnt) and (o[n:] == SENT).all()
    assert np.array_equal(f[:n], (cnt > 0).astype(np.int8)) and (f[n:] == SENT).all()
    off = np.concatenate([[0], np.cumsum(cnt.astype(np.int64))])
    ids, seg, lout = raw_list(c.scene, ctx, planes, n, off)
    assert np.array_equal(lout[:n].view(U), cnt) and (lout[n:] == SENT).all()
    assert (ids[off[-1]:] == SENT).all() and (seg[off[-1]:] == SENT_U).all()
    for i in range(n):
        assert np.array_equal(by_id(seg[off[i]:off[i + 1]]), c.exp["segs"][i]), i
        assert np.array_equal(np.sort(ids[off[i]:off[i + 1]]).view(U), c.exp["ids"][i]), i


# ---- 6. LIST segmentation: exact, one short, a fixed stride ------------------------------------------------
def test_list_segments_exact_short_and_strided(ctx):
    import torch
    c = case(ctx, "torus")
    n = c.pts.shape[0]
    cnt = c.exp["count"].astype(np.int64)
    planes = torch.from_numpy(pack(c.pts, c.nrm)).to(torch.device("cuda", ctx.device))
    exact = np.concatenate([[0], np.cumsum(cnt)])
    short = np.concatenate([[0], np.cumsum(np.maximum(cnt - 1, 0))])
    stride = np.arange(n + 1) * 4
    full_ids, full_seg, full_out = raw_list(c.scene, ctx, planes, n, exact)
    for name, off in (("exact", exact), ("one short", short), ("stride 4", stride)):
        ids, seg, out = raw_list(c.scene, ctx, planes, n, off)
        assert np.array_equal(out[:n].view(U), c.exp["count"]), name  # the true count, whatever fitted
        assert (out[n:] == SENT).all() and (ids[off[-1]:] == SENT).all() and (seg[off[-1]:] == SENT_U).all(), name
        for i in range(n):
            k = min(int(cnt[i]), int(off[i + 1] - off[i]))
            # the first k entries of the traversal's order (the exact run's segment), then an untouched tail
            assert np.array_equal(ids[off[i]:off[i] + k], full_ids[exact[i]:exact[i] + k]), (name, i)
            assert np.array_equal(seg[off[i]:off[i] + k], full_seg[exact[i]:exact[i] + k]), (name, i)
            assert (ids[off[i] + k:off[i + 1]] == SENT).all() and (seg[off[i] + k:off[i + 1]] == SENT_U).all(), (name, i)
    for i in range(n):  # and the exact run holds each plane's set
        assert np.array_equal(by_id(full_seg[exact[i]:exact[i + 1]]), c.exp["segs"][i]), i
    assert (cnt > 4).any() and (cnt < 4).any()
    # a null out_dev: the same contents
    ids2, seg2, _ = raw_list(c.scene, ctx, planes, n, exact, out=False)
    assert np.array_equal(ids2, full_ids) and np.array_equal(seg2, full_seg)


def test_list_order_is_the_same_on_every_call_and_grid(ctx):
    import torch
    c = case(ctx, "torus")
    n = c.pts.shape[0]
    exact = np.concatenate([[0], np.cumsum(c.exp["count"].astype(np.int64))])
    planes = torch.from_numpy(pack(c.pts, c.nrm)).to(torch.device("cuda", ctx.device))
    first = raw_list(c.scene, ctx, planes, n, exact)
    again = raw_list(c.scene, ctx, planes, n, exact)
    assert all(np.array_equal(x, y) for x, y in zip(first, again))
    small = beam.Context(device=0, params={"trace_grid": 2})  # 8 waves stride over the batches
    scene, keep = build(small, c.meshes)
    other = raw_list(scene, small, planes, n, exact)
    assert all(np.array_equal(x, y) for x, y in zip(first, other))
    assert_planes(scene, small, c.pts, c.nrm, c.exp, "two workgroups", modes=("count", "any"))
    scene.destroy()
    small.close()


# ---- 7. ANY; invalid planes ------------------------------------------------------------------------------
def test_any_equals_count_above_zero_and_stops_early(ctx):
    c = case(ctx, "suzanne")
    cnt = c.scene.sectionPlanes(c.pts, c.nrm, mode="count", counters=True)
    hit = c.scene.sectionPlanes(c.pts, c.nrm, mode="any", counters=True)
    assert np.array_equal(hit["any"], cnt["count"] > 0)
    assert int(hit["counters"][2]) == int((cnt["count"] > 0).sum()) and int(cnt["counters"][2]) == int(cnt["count"].sum())
    n = c.pts.shape[0]
    print("suzanne, per plane: " + ", ".join(f"{name} {int(r['counters'][0]) / n:.1f} node records, "
                                             f"{int(r['counters'][1]) / n:.1f} triangle tests"
                                             for name, r in (("count", cnt), ("any", hit))))
    assert int(hit["counters"][0]) <= int(cnt["counters"][0]) and int(hit["counters"][1]) <= int(cnt["counters"][1])
    assert int(hit["counters"][1]) < int(cnt["counters"][1])


def test_invalid_planes_find_nothing(ctx):
    c = case(ctx, "torus")
    pts, nrm = c.pts.copy(), c.nrm.copy()
    n = pts.shape[0]
    sel = np.arange(1, n, 3)
    for j, i in enumerate(sel):
        pts[i], nrm[i] = F(ps.INVALID[j % len(ps.INVALID)][0]), F(ps.INVALID[j % len(ps.INVALID)][1])
    invalid = np.zeros(n, bool)
    invalid[sel] = True
    exp = brute_planes(pts, nrm, c.verts)
    assert (exp["count"][invalid] == 0).all() and np.array_equal(exp["count"][~invalid], c.exp["count"][~invalid])
    assert_planes(c.scene, ctx, pts, nrm, exp, "invalid planes")
    for mode in ("count", "any", "list"):
        alone = c.scene.sectionPlanes(pts[invalid], nrm[invalid], mode=mode, counters=True)
        assert [int(x) for x in alone["counters"]] == [0, 0, 0, 0], mode  # invalid planes count nothing
        assert not alone["any" if mode == "any" else "count"].any()


# ---- 8. the stack's overflow area ------------------------------------------------------------------------
def test_deep_chain_uses_the_overflow_area():
    """tests/deep_scenes.py's chain under a plane that crosses every triangle of it: nothing is pruned, so the
    siblings of the whole descent wait on the stack."""
    _, dup, leaf = ds.scene_of("deep")
    dctx = beam.Context(device=0, leaf_size=leaf)
    meshes = ds.deep_meshes(dup)
    verts = tri_vertices(meshes)
    rng = np.random.default_rng(9)
    pts = np.concatenate([F([[100, 0, 0]]), F(rng.uniform(-1000, 2000, (40, 3)))])
    nrm = np.concatenate([F([[1, 0, 0]]), F(rng.normal(size=(40, 3)))])
    exp = brute_planes(pts, nrm, verts)
    assert exp["count"][0] == verts.shape[0]
    scene, keep = build(dctx, meshes)
    for mode in ("count", "list"):
        res = scene.sectionPlanes(pts, nrm, mode=mode, counters=True)
        deepest = int(res["counters"][3])
        print(f"deep chain, {mode}: deepest stack {deepest} entries (LDS holds {QUAD_LDS})")
        assert deepest >= QUAD_LDS + 1, f"the overflow path did not run: deepest stack {deepest}"
        assert deepest <= ds.MAX_STACK
        assert np.array_equal(res["count"], exp["count"])
    assert_planes(scene, dctx, pts, nrm, exp, "deep chain")
    scene.destroy()
    dctx.close()


# ---- 9. other scene states ---------------------------------------------------------------------------------
def test_after_a_device_vertex_upload_and_refit(ctx):
    import torch
    c = case(ctx, "torus")
    dev = torch.device("cuda", ctx.device)
    scene = beam.IScene.create(ctx)
    meshes = beam.upload_meshes(ctx, scene, c.meshes)
    scene.updateGPUScene()
    p = np.asarray(c.meshes[0]["pos"], F).reshape(-1, 3)
    q = p.copy()  # scaled and sheared
    q[:, 0] = p[:, 0] * F(1.25) + p[:, 1] * F(0.5)
    q[:, 1] = p[:, 1] * F(0.75)
    q[:, 2] = p[:, 2] * F(1.5) + p[:, 0] * F(0.25)
    t = torch.from_numpy(q).to(dev)
    torch.cuda.synchronize()
    assert meshes[0].setVertexData(t, q.shape[0], 3, beam.VERTEX_DATA_POSITION) == 0
    scene.refitGPUScene()
    moved = [dict(c.meshes[0], pos=q)]
    verts = tri_vertices(moved)
    pts, nrm, groups = ps.designed_planes(verts, seed=13)
    exp = brute_planes(pts, nrm, verts)
    old = brute_planes(pts, nrm, c.verts)  # the results follow the new positions
    assert (exp["count"][groups["vertex"]] > 0).all() and np.mean(old["count"] != exp["count"]) > 0.3
    assert_planes(scene, ctx, pts, nrm, exp, "after upload and refit")
    scene.destroy()


def test_instanced_scene(ctx):
    from test_instances_abi import MIRROR, rotation, xform_mesh
    c = case(ctx, "torus")
    base = c.meshes[0]
    x_rot = rotation((1, 2, 3), 0.7, (7.5, -0.25, 2.0))
    x_mir = np.array(MIRROR, F)
    x_mir[:, 3] = F([-7.25, 0.5, -1.0])
    scene = beam.IScene.create(ctx)
    mesh = beam.upload_meshes(ctx, scene, [base])[0]  # entry 0: the plain one
    assert scene.addInstance(mesh, x_rot) == 1
    assert scene.addInstance(mesh, x_mir) == 2
    scene.updateGPUScene()
    pre = [base, xform_mesh(x_rot, base), xform_mesh(x_mir, base)]  # the header's transform arithmetic, restated
    verts = tri_vertices(pre)
    pts, nrm, groups = ps.designed_planes(verts, seed=14)
    exp = brute_planes(pts, nrm, verts)
    n1 = c.verts.shape[0]
    assert {int(g) // n1 for a in exp["ids"] for g in a} == {0, 1, 2}
    assert_planes(scene, ctx, pts, nrm, exp, "instances")
    for i in range(pts.shape[0]):  # each copy is closed, the mirrored one too: the loops close
        assert ps.loop_closure(exp["segs"][i]), i
    scene.destroy()


@pytest.mark.parametrize("leaf", [1, 2, 16])
def test_leaf_sizes(leaf):
    lctx = beam.Context(device=0, leaf_size=leaf)
    meshes, verts, pts, nrm, groups = ps.icosphere_case()
    exp = brute_planes(pts, nrm, verts)
    scene, keep = build(lctx, meshes)
    assert_planes(scene, lctx, pts, nrm, exp, f"leaf size {leaf}")
    scene.destroy()
    lctx.close()


def test_repeated_device_context_queries_on_the_root(ctx):
    c = case(ctx, "icosphere")
    multi = beam.Context(devices=[0, 0])
    scene, keep = build(multi, c.meshes)
    assert_planes(scene, multi, c.pts, c.nrm, c.exp, "devices=[0, 0]", modes=("count", "any", "segments"))
    scene.destroy()
    multi.close()


# ---- 10. the Python layer ----------------------------------------------------------------------------------
def test_slice_stack_equals_the_restated_planes(ctx):
    c = case(ctx, "torus")
    origin, normal = F([0.1, -0.2, -0.9]), F([0.05, 0.1, 1.0])
    heights = F(np.linspace(-0.2, 2.0, 37))
    pts = origin[None, :] + heights[:, None] * normal[None, :]  # the docstring's statements
    assert pts.dtype == F
    nrm = np.ascontiguousarray(np.broadcast_to(normal, pts.shape))
    exp = brute_planes(pts, nrm, c.verts)
    assert 20 < int((exp["count"] > 0).sum()) < 37
    off, ids, a, b = c.scene.sliceStack(origin, normal, heights)
    assert np.array_equal(np.diff(off.astype(np.int64)), exp["count"])
    for i, want in enumerate(exp["segs"]):
        sl = slice(int(off[i]), int(off[i + 1]))
        order = np.argsort(ids[sl], kind="stable")
        assert np.array_equal(ids[sl][order], want[:, 3])
        assert np.array_equal(a[sl][order].view(U), want[:, 0:3]) and np.array_equal(b[sl][order].view(U), want[:, 4:7])
        lp, ch = beam.chainSegments(a[sl], b[sl])
        assert not ch and (len(lp) >= 1) == (exp["count"][i] > 0)
    assert np.array_equal(c.scene.sliceStack(origin, normal, heights, mode="count")["count"], exp["count"])


def test_torch_chain_into_hit_attributes(ctx):
    """Planes -> sectionPlanes(mode="segments") -> the ids as bm_hit records -> hitAttributes(BM_ATTR_MESH_FACE) on
    one stream: which mesh and face each cut triangle is."""
    import torch
    dev = torch.device("cuda", 0)
    tctx = beam.Context(device=0, stream=torch.cuda.current_stream(dev).cuda_stream)
    tor, ball = ps.torus(), ps.icosphere(centre=(0.5, 0.25, -0.5))
    meshes = tor + ball  # two meshes: the owner is not always mesh 0
    verts = tri_vertices(meshes)
    pts, nrm, groups = ps.designed_planes(verts, seed=15)
    exp = brute_planes(pts, nrm, verts)
    scene, keep = build(tctx, meshes)
    off, ids, a, b = scene.sectionPlanes(torch.from_numpy(pts).to(dev), torch.from_numpy(nrm).to(dev), mode="segments")
    assert ids.is_cuda and ids.dtype == torch.int32 and off.shape == (pts.shape[0] + 1,) and a.is_cuda and b.is_cuda
    hits = torch.zeros((ids.shape[0], 4), dtype=torch.float32, device=dev)
    hits.view(torch.int32)[:, 3] = ids
    (face,) = scene.hitAttributes(hits, [(beam.ATTR_MESH_FACE, 2)])
    packed = torch.from_numpy(pack(pts, nrm)).to(dev)
    hit = scene.sectionPlanes(packed, mode="any")["any"]
    torch.cuda.synchronize()
    off, ids = off.cpu().numpy().view(U), ids.cpu().numpy().view(U)
    a, b = a.cpu().numpy(), b.cpu().numpy()
    assert np.array_equal(np.diff(off.astype(np.int64)), exp["count"])
    for i, want in enumerate(exp["segs"]):
        sl = slice(int(off[i]), int(off[i + 1]))
        order = np.argsort(ids[sl], kind="stable")
        assert np.array_equal(ids[sl][order], want[:, 3]), i
        assert np.array_equal(a[sl][order].view(U), want[:, 0:3]) and np.array_equal(b[sl][order].view(U), want[:, 4:7]), i
    n1 = 768
    g = ids.astype(np.int64)
    assert np.array_equal(face.cpu().numpy(), np.stack([(g >= n1).astype(np.int64), np.where(g >= n1, g - n1, g)], axis=1))
    assert set((g >= n1).tolist()) == {False, True}
    assert np.array_equal(hit.cpu().numpy(), exp["count"] > 0)
    scene.destroy()
    tctx.close()


# ---- 11. errors ----------------------------------------------------------------------------------------------
def test_errors(ctx):
    import torch
    c = case(ctx, "torus")
    dev = torch.device("cuda", ctx.device)
    n = 64
    planes = torch.zeros((n + 1, 8), dtype=torch.float32, device=dev)
    out = torch.zeros((n + 2,), dtype=torch.int32, device=dev)
    off = torch.zeros((n + 2,), dtype=torch.int32, device=dev)
    ids = torch.zeros((64,), dtype=torch.int32, device=dev)
    segs = torch.zeros((66, 8), dtype=torch.float32, device=dev)
    torch.cuda.synchronize()
    pp, op, fp, ip, sp = planes.data_ptr(), out.data_ptr(), off.data_ptr(), ids.data_ptr(), segs.data_ptr()
    unbuilt = beam.IScene.create(ctx)
    assert unbuilt.sectionPlanesDevice(pp, n, COUNT, op) == _lib.ERROR_NOT_BUILT
    unbuilt.destroy()
    s = c.scene
    assert s.sectionPlanesDevice(pp, n, COUNT, op) == 0 and s.sectionPlanesDevice(pp, n, ANY, op) == 0
    assert s.sectionPlanesDevice(pp, n, LIST, op, fp, ip, sp) == 0 and s.sectionPlanesDevice(pp, n, LIST, 0, fp, ip) == 0
    assert s.sectionPlanesDevice(pp, n, LIST, 0, fp, 0, sp) == 0
    assert s.sectionPlanesDevice(0, 0, COUNT, 0) == 0 and s.sectionPlanesDevice(0, 0, LIST, 0) == 0  # n = 0: nothing read
    for mode in (3, 4, 0x80000000):
        assert s.sectionPlanesDevice(pp, n, mode, op, fp, ip, sp) == BAD
    for flags in (1, 2, 0x80000000):
        assert s.sectionPlanesDevice(pp, n, COUNT, op, flags=flags) == BAD
    assert s.sectionPlanesDevice(0, n, COUNT, op) == BAD and s.sectionPlanesDevice(pp, n, COUNT, 0) == BAD
    assert s.sectionPlanesDevice(pp, n, ANY, 0) == BAD
    assert s.sectionPlanesDevice(pp, n, LIST, op, 0, ip, sp) == BAD
    assert s.sectionPlanesDevice(pp, n, LIST, op, fp, 0, 0) == BAD  # LIST with neither ids nor segments
    off_b = planes.view(-1)[1:].data_ptr()            # 4 bytes in
    byte = lambda t: t.view(torch.int8)[1:].data_ptr()  # 1 byte in
    assert off_b == pp + 4 and byte(out) == op + 1
    assert s.sectionPlanesDevice(off_b, n, COUNT, op) == BAD
    assert s.sectionPlanesDevice(planes.view(-1)[4:].data_ptr(), n, COUNT, op) == 0  # planes are 16-byte aligned
    assert s.sectionPlanesDevice(pp, n, COUNT, byte(out)) == BAD
    assert s.sectionPlanesDevice(pp, n, ANY, byte(out)) == 0                        # the byte plane: any address
    assert s.sectionPlanesDevice(pp, n, LIST, byte(out), fp, ip, sp) == BAD
    assert s.sectionPlanesDevice(pp, n, LIST, op, byte(off), ip, sp) == BAD
    assert s.sectionPlanesDevice(pp, n, LIST, op, fp, byte(ids), sp) == BAD
    assert s.sectionPlanesDevice(pp, n, LIST, op, fp, ip, segs.view(-1)[1:].data_ptr()) == BAD  # segments: 16 bytes
    assert s.sectionPlanesDevice(pp, n, LIST, op, fp, ip, segs.view(-1)[4:].data_ptr()) == 0
    assert s.sectionPlanesDevice(pp, n, LIST, out[1:].data_ptr(), off[1:].data_ptr(), ids[1:].data_ptr()) == 0
    assert s.sectionPlanesDevice(pp, n, COUNT, op, byte(off), byte(ids), byte(segs)) == 0  # COUNT ignores them
    counters = np.zeros(4, np.uint64)
    assert s.sectionPlanesDevice(pp, n, 3, op, counters=counters) == BAD
    assert s.ctx.lib.bm_scene_section_planes_counters(s.h, pp, n, COUNT, 0, op, None, None, None, None) == BAD
    assert s.ctx.lib.bm_scene_section_planes(None, pp, n, COUNT, 0, op, None, None, None) == BAD  # a null handle
    ctx.sync()
    with pytest.raises(beam.BeamError):
        s.sectionPlanes(np.zeros((4, 3), F), np.ones((4, 3), F), mode="all")
    # a mesh added since the build: the meshes are no longer the build's
    stale = beam.IScene.create(ctx)
    keep = beam.upload_meshes(ctx, stale, c.meshes)
    stale.updateGPUScene()
    more = beam.upload_meshes(ctx, stale, ps.icosphere())
    assert stale.sectionPlanesDevice(pp, n, COUNT, op) == _lib.ERROR_NOT_BUILT
    stale.destroy()
    tiny = [{"pos": F([[0, 0, 1], [1, 0, 1], [0, 1, 1]]), "nrm": F([[0, 0, 1]] * 3), "idx": np.uint32([0, 1, 2])}]
    # (a BVH8 context exists in A/B builds only: the product library refuses to create one)
    for kw in ({"reference_kd": True}, {"reference_hash": True}, {"bvh_width": 2}):
        other = beam.Context(device=0, **kw)
        sc, keep = build(other, tiny)
        for mode in (COUNT, ANY, LIST):
            assert sc.sectionPlanesDevice(pp, n, mode, op, fp, ip, sp) == BAD, kw
        assert sc.sectionPlanesDevice(pp, n, COUNT, op, counters=counters) == BAD, kw
        sc.destroy()
        other.close()
