"""GPU checks of box overlap queries (bm_scene_overlap_boxes): the triangles that intersect each box of a batch.

Every comparison is exact against brute_boxes of tests/test_boxes_abi.py: the header's triangle/box function
restated in numpy float32 and evaluated for every triangle and every box. The traversal prunes, the brute force
does not. LIST segments are compared as sorted sets with their counts. A reference is computed once per scene
and box set and left unchanged. No expected value comes from the library.
"""
from types import SimpleNamespace

import numpy as np
import pytest

import deep_scenes as ds
from raytracercuda_amd import _lib, beam, scenes
from test_boxes_abi import (F, RULES, SHIFTS, bounds, brute_boxes, centroid_boxes, grid_boxes, rule_scene,
                            sliver_boxes, sliver_meshes, suzanne_sets, translated, tri_vertices)

pytestmark = pytest.mark.gpu

COUNT, ANY, LIST = _lib.BOXES_COUNT, _lib.BOXES_ANY, _lib.BOXES_LIST
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


def assert_boxes(scene, ctr, half, exp, what="", modes=("count", "any", "list")):
    """All of scene.overlapBoxes' modes over the boxes equal brute_boxes' answer exp."""
    n = ctr.shape[0]
    if "count" in modes:
        res = scene.overlapBoxes(ctr, half, mode="count")
        bad = np.flatnonzero(res["count"] != exp["count"])
        assert bad.size == 0, f"{what}: count differs on {bad.size} of {n} boxes, first {bad[:5]}"
    if "any" in modes:
        res = scene.overlapBoxes(ctr, half, mode="any")
        assert res["any"].dtype == bool and np.array_equal(res["any"], exp["count"] > 0), (what, "any")
    if "list" in modes:
        res = scene.overlapBoxes(ctr, half, mode="list")
        assert np.array_equal(res["count"], exp["count"]), (what, "list count")
        assert res["offsets"].shape == (n + 1,) and res["offsets"][0] == 0
        assert np.array_equal(np.diff(res["offsets"].astype(np.int64)), exp["count"]), (what, "offsets")
        assert res["ids"].shape == (int(exp["count"].sum()),)
        for i, (got, want) in enumerate(zip(segments(res), exp["ids"])):
            assert np.array_equal(got, want), (what, "ids of box", i)


def random_boxes(rng, n, lo, hi):
    """n boxes about [lo, hi]: centres inside and a little around it, half-sizes from tiny to the whole extent."""
    ext = (hi - lo).astype(np.float64)
    ctr = rng.uniform(lo - 0.2 * ext, hi + 0.2 * ext, (n, 3))
    half = ext.max() * 10 ** rng.uniform(-3, 0, (n, 1)) * rng.uniform(0.3, 1.0, (n, 3))
    return F(ctr), F(half)


_CASES = {}


def case(ctx, name):
    """Meshes, GPU scene and, per box set, the boxes with brute_boxes' answer — made once per module run.
    suzanne: the 8^3 grid over its bounding box and the boxes at every 16th triangle's centroid; bunny: the 6^3
    grid over its bounding box."""
    if name not in _CASES:
        meshes = scenes.load_mesh(name)
        verts = tri_vertices(meshes)
        if name == "suzanne":
            sets = suzanne_sets()[1]
        else:
            sets = {"grid": grid_boxes(*bounds(verts), (6, 6, 6))}
        exp = {}
        for key, (c, h) in sets.items():
            exp[key] = brute_boxes(c, h, verts)
            exp[key]["count"].setflags(write=False)
        scene, keep = build(ctx, meshes)
        _CASES[name] = SimpleNamespace(meshes=meshes, verts=verts, scene=scene, keep=keep, sets=sets, exp=exp)
    return _CASES[name]


def teardown_module(module):
    for k in _CASES.values():
        k.scene.destroy()
    _CASES.clear()


# ---- 1. the rules ----------------------------------------------------------------------------------------
def test_rule_cases(ctx):
    verts, ctr, half = rule_scene()
    exp = brute_boxes(ctr, half, verts)
    scene, keep = build(ctx, soup(verts))
    assert_boxes(scene, ctr, half, exp, "rules")
    res = scene.overlapBoxes(ctr, half, mode="list")
    for i, (r, got) in enumerate(zip(RULES, segments(res))):
        assert (i in got.tolist()) == r[4], r[0]
    assert (res["count"][len(RULES):] == 0).all()  # the invalid boxes
    scene.destroy()


# ---- 2. tiny scenes: the empty tree, the one-leaf root, a full leaf, a leaf plus one, several records ------
@pytest.mark.parametrize("ntri", [0, 1, 2, 4, 5, 17])
def test_tiny_scenes(ctx, ntri):
    rng = np.random.default_rng(300 + ntri)
    verts = F(rng.uniform(-1, 1, (ntri, 1, 3)) + rng.uniform(-0.4, 0.4, (ntri, 3, 3)))
    scene, keep = build(ctx, soup(verts) if ntri else [])
    ctr, half = random_boxes(rng, 203, F([-1.4] * 3), F([1.4] * 3))
    ctr[0], half[0] = 0, 4  # holds everything
    exp = brute_boxes(ctr, half, verts)
    assert exp["count"][0] == ntri and (ntri == 0 or 0 < int((exp["count"] > 0).sum()) < 203)
    assert_boxes(scene, ctr, half, exp, f"{ntri} triangles")
    res = scene.overlapBoxes(ctr, half, mode="count", counters=True)
    assert int(res["counters"][2]) == int(exp["count"].sum())
    if ntri == 0:  # a built scene with no triangles: zeros, nothing fetched or tested
        assert [int(x) for x in res["counters"]] == [0, 0, 0, 0] and (res["count"] == 0).all()
    scene.destroy()


# ---- 3. meshes -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["count", "any", "list"])
@pytest.mark.parametrize("which", ["grid", "centroid"])
def test_suzanne(ctx, which, mode):
    c = case(ctx, "suzanne")
    ctr, half = c.sets[which]
    cnt = c.exp[which]["count"].astype(np.int64)
    if which == "grid":
        assert ctr.shape[0] == 512 and np.mean(cnt == 0) >= 0.40 and np.mean(cnt > 64) >= 0.08
    else:
        assert ctr.shape[0] == 968 and (cnt >= 1).all()
    assert_boxes(c.scene, ctr, half, c.exp[which], f"suzanne {which}", modes=(mode,))


def test_any_equals_count_above_zero_and_stops_early(ctx):
    c = case(ctx, "suzanne")
    ctr, half = c.sets["grid"]
    cnt = c.scene.overlapBoxes(ctr, half, mode="count", counters=True)
    hit = c.scene.overlapBoxes(ctr, half, mode="any", counters=True)
    assert np.array_equal(hit["any"], cnt["count"] > 0)
    assert int(hit["counters"][2]) == int((cnt["count"] > 0).sum()) and int(cnt["counters"][2]) == int(cnt["count"].sum())
    n = ctr.shape[0]
    print("suzanne grid, per box: " + ", ".join(f"{name} {int(r['counters'][0]) / n:.1f} node records, "
                                                f"{int(r['counters'][1]) / n:.1f} triangle tests"
                                                for name, r in (("count", cnt), ("any", hit))))
    assert int(hit["counters"][0]) <= int(cnt["counters"][0]) and int(hit["counters"][1]) < int(cnt["counters"][1])


def test_bunny_grid(ctx):
    c = case(ctx, "bunny")
    ctr, half = c.sets["grid"]
    assert ctr.shape[0] == 216 and 0 < int((c.exp["grid"]["count"] == 0).sum()) < 216
    assert_boxes(c.scene, ctr, half, c.exp["grid"], "bunny grid")


# ---- 4. large coordinates and reconstructed vertices: nothing the padding must cover is lost ----------------
@pytest.mark.parametrize("shift", SHIFTS)
def test_translated_suzanne(ctx, shift):
    moved = translated(scenes.load_mesh("suzanne"), shift)
    verts = tri_vertices(moved)
    gc, gh = grid_boxes(*bounds(verts), (8, 8, 8))
    cc, ch = centroid_boxes(verts, every=32)
    ctr, half = np.concatenate([gc, cc]), np.concatenate([gh, ch])
    exp = brute_boxes(ctr, half, verts)
    assert (exp["count"][512:] >= 1).all() and np.mean(exp["count"][:512] == 0) >= 0.40
    scene, keep = build(ctx, moved)
    assert_boxes(scene, ctr, half, exp, f"suzanne + {shift}")
    scene.destroy()


def test_slivers_across_magnitudes(ctx):
    meshes = sliver_meshes()
    verts = tri_vertices(meshes)
    ctr, half = sliver_boxes(verts)
    exp = brute_boxes(ctr, half, verts)
    assert 0.1 < np.mean(exp["count"] > 0) < 0.9 and exp["count"].max() == verts.shape[0]
    scene, keep = build(ctx, meshes)
    assert_boxes(scene, ctr, half, exp, "slivers")
    scene.destroy()


# ---- 5. one box around everything --------------------------------------------------------------------------
def test_one_box_holding_the_scene(ctx):
    c = case(ctx, "suzanne")
    lo, hi = bounds(c.verts)
    ctr, half = ((lo + hi) * F(0.5))[None], ((hi - lo) * F(0.5) + F(1))[None]
    ntri = c.verts.shape[0]
    assert brute_boxes(ctr, half, c.verts)["count"].tolist() == [ntri]
    res = c.scene.overlapBoxes(ctr, half, mode="count", counters=True)
    assert res["count"].tolist() == [ntri]
    assert int(res["counters"][1]) == ntri and int(res["counters"][2]) == ntri  # every leaf once, nothing twice
    lst = c.scene.overlapBoxes(ctr, half, mode="list")
    assert np.array_equal(np.sort(lst["ids"]), np.arange(ntri, dtype=np.uint32))
    assert c.scene.overlapBoxes(ctr, half, mode="any")["any"].tolist() == [True]


# ---- 6. LIST segmentation: exact, one short, a fixed stride ------------------------------------------------
def raw_list(scene, ctx, boxes_dev, n, offsets, tail=64):
    """One raw LIST call with sentinel-filled ids and counts; returns (ids with the tail, counts with the tail)."""
    import torch
    dev = boxes_dev.device
    off = torch.from_numpy(np.ascontiguousarray(offsets, np.int32)).to(dev)
    ids = torch.full((int(offsets[-1]) + tail,), SENT, dtype=torch.int32, device=dev)
    out = torch.full((n + tail,), SENT, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    assert scene.overlapBoxesDevice(boxes_dev.data_ptr(), n, LIST, out.data_ptr(), off.data_ptr(), ids.data_ptr()) == 0
    ctx.sync()
    return ids.cpu().numpy(), out.cpu().numpy()


def pack(ctr, half):
    b = np.zeros((ctr.shape[0], 8), F)
    b[:, 0:3], b[:, 4:7] = ctr, half
    b.view(np.uint32)[:, 3], b.view(np.uint32)[:, 7] = 0xDEADBEEF, 0x7FC00000  # the pad words are ignored
    return b


def test_list_segments_exact_short_and_strided(ctx):
    import torch
    c = case(ctx, "suzanne")
    ctr, half = c.sets["grid"]
    exp = c.exp["grid"]
    n = ctr.shape[0]
    cnt = exp["count"].astype(np.int64)
    boxes = torch.from_numpy(pack(ctr, half)).to(torch.device("cuda", ctx.device))
    exact = np.concatenate([[0], np.cumsum(cnt)])
    short = np.concatenate([[0], np.cumsum(np.maximum(cnt - 1, 0))])
    stride = np.arange(n + 1) * 4
    full_ids, full_out = raw_list(c.scene, ctx, boxes, n, exact)
    for name, off in (("exact", exact), ("one short", short), ("stride 4", stride)):
        ids, out = raw_list(c.scene, ctx, boxes, n, off)
        assert np.array_equal(out[:n].view(np.uint32), exp["count"]), name  # the true count, whatever fitted
        assert (out[n:] == SENT).all() and (ids[off[-1]:] == SENT).all(), name  # nothing past the ends
        for i in range(n):
            seg = ids[off[i]:off[i + 1]]
            k = min(int(cnt[i]), seg.size)
            # the first k ids of the traversal's order (the exact run's segment), then an untouched tail
            assert np.array_equal(seg[:k], full_ids[exact[i]:exact[i] + k]), (name, i)
            assert (seg[k:] == SENT).all(), (name, i)
    for i in range(n):  # and the exact run holds each box's set
        assert np.array_equal(np.sort(full_ids[exact[i]:exact[i + 1]]).view(np.uint32), exp["ids"][i]), i
    assert (short[1:] - short[:-1] < cnt).sum() == int((cnt > 0).sum()) and (cnt > 4).any() and (cnt < 4).any()
    # a null out_dev: the ids alone
    dev = boxes.device
    ids2 = torch.full((int(exact[-1]) + 64,), SENT, dtype=torch.int32, device=dev)
    off = torch.from_numpy(exact.astype(np.int32)).to(dev)
    torch.cuda.synchronize()
    assert c.scene.overlapBoxesDevice(boxes.data_ptr(), n, LIST, 0, off.data_ptr(), ids2.data_ptr()) == 0
    ctx.sync()
    assert np.array_equal(ids2.cpu().numpy(), full_ids)


def test_list_order_is_the_same_on_every_call_and_grid(ctx):
    c = case(ctx, "suzanne")
    ctr, half = c.sets["grid"]
    first = c.scene.overlapBoxes(ctr, half, mode="list")
    again = c.scene.overlapBoxes(ctr, half, mode="list")
    assert np.array_equal(first["ids"], again["ids"]) and np.array_equal(first["offsets"], again["offsets"])
    small = beam.Context(device=0, params={"trace_grid": 2})  # 8 waves stride over the 32 batches
    scene, keep = build(small, c.meshes)
    other = scene.overlapBoxes(ctr, half, mode="list")
    assert np.array_equal(first["ids"], other["ids"]) and np.array_equal(first["offsets"], other["offsets"])
    assert_boxes(scene, ctr, half, c.exp["grid"], "two workgroups", modes=("count", "any"))
    scene.destroy()
    small.close()


# ---- 7. invalid boxes ------------------------------------------------------------------------------------
def test_invalid_boxes_find_nothing(ctx):
    c = case(ctx, "suzanne")
    ctr, half = (a.copy() for a in c.sets["centroid"])
    n = ctr.shape[0]
    sel = np.arange(3, n, 7)
    kind = (sel // 7) % 10
    for ax in range(3):
        ctr[sel[kind == ax], ax] = (np.nan, np.inf, -np.inf)[ax]
        half[sel[kind == 3 + ax], ax] = (np.nan, np.inf, -1.0)[ax]
    half[sel[kind == 6], 1] = -1e-30
    half[sel[kind == 7]] = np.nan
    ctr[sel[kind == 8]] = np.inf
    half[sel[kind == 9], 0] = -np.inf
    invalid = np.zeros(n, bool)
    invalid[sel] = True
    exp = brute_boxes(ctr, half, c.verts)
    assert (exp["count"][invalid] == 0).all() and (exp["count"][~invalid] >= 1).all()
    assert np.array_equal(exp["count"][~invalid], c.exp["centroid"]["count"][~invalid])
    assert_boxes(c.scene, ctr, half, exp, "invalid boxes")
    for mode in ("count", "any", "list"):
        alone = c.scene.overlapBoxes(ctr[invalid], half[invalid], mode=mode, counters=True)
        assert [int(x) for x in alone["counters"]] == [0, 0, 0, 0], mode  # invalid boxes count nothing
        assert not alone["any" if mode == "any" else "count"].any()


# ---- 8. batch edges --------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 15, 16, 17, 33])
def test_batch_edges_write_nothing_past_n(ctx, n):
    import torch
    c = case(ctx, "suzanne")
    ctr, half = c.sets["centroid"]
    exp = c.exp["centroid"]
    dev = torch.device("cuda", ctx.device)
    boxes = torch.from_numpy(pack(ctr[:n], half[:n])).to(dev)
    cnt = exp["count"][:n]
    out = torch.full((n + 64,), SENT, dtype=torch.int32, device=dev)
    flag = torch.full((n + 64,), SENT, dtype=torch.int8, device=dev)
    torch.cuda.synchronize()
    assert c.scene.overlapBoxesDevice(boxes.data_ptr(), n, COUNT, out.data_ptr()) == 0
    assert c.scene.overlapBoxesDevice(boxes.data_ptr(), n, ANY, flag.data_ptr()) == 0
    ctx.sync()
    o, f = out.cpu().numpy(), flag.cpu().numpy()
    assert np.array_equal(o[:n].view(np.uint32), cnt) and (o[n:] == SENT).all()
    assert np.array_equal(f[:n], (cnt > 0).astype(np.int8)) and (f[n:] == SENT).all()
    off = np.concatenate([[0], np.cumsum(cnt.astype(np.int64))])
    ids, lout = raw_list(c.scene, ctx, boxes, n, off)
    assert np.array_equal(lout[:n].view(np.uint32), cnt) and (lout[n:] == SENT).all() and (ids[off[-1]:] == SENT).all()
    for i in range(n):
        assert np.array_equal(np.sort(ids[off[i]:off[i + 1]]).view(np.uint32), exp["ids"][i]), i


# ---- 9. the stack's overflow area ------------------------------------------------------------------------
def test_deep_chain_uses_the_overflow_area():
    """tests/deep_scenes.py's chain under a box that holds it: nothing is pruned, so the siblings of the whole
    descent wait on the stack."""
    _, dup, leaf = ds.scene_of("deep")
    dctx = beam.Context(device=0, leaf_size=leaf)
    meshes = ds.deep_meshes(dup)
    verts = tri_vertices(meshes)
    lo, hi = bounds(verts)
    rng = np.random.default_rng(9)
    rc, rh = random_boxes(rng, 70, lo, hi)
    ctr = np.concatenate([((lo + hi) * F(0.5))[None], rc])
    half = np.concatenate([((hi - lo) * F(0.5) + F(1))[None], rh])
    exp = brute_boxes(ctr, half, verts)
    assert exp["count"][0] == verts.shape[0]
    scene, keep = build(dctx, meshes)
    for mode in ("count", "list"):
        res = scene.overlapBoxes(ctr, half, mode=mode, counters=True)
        deepest = int(res["counters"][3])
        print(f"deep chain, {mode}: deepest stack {deepest} entries (LDS holds {QUAD_LDS})")
        assert deepest >= QUAD_LDS + 1, f"the overflow path did not run: deepest stack {deepest}"
        assert deepest <= ds.MAX_STACK
        assert np.array_equal(res["count"], exp["count"])
    assert_boxes(scene, ctr, half, exp, "deep chain")
    scene.destroy()
    dctx.close()


# ---- 10. other scene states --------------------------------------------------------------------------------
def test_query_after_refit(ctx):
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
        assert m.setVertexData(mv["pos"], mv["pos"].shape[0], 3, beam.VERTEX_DATA_POSITION) == 0
    scene.refitGPUScene()
    verts = tri_vertices(moved)
    gc, gh = grid_boxes(*bounds(verts), (6, 6, 6))
    cc, ch = centroid_boxes(verts, every=64)
    ctr, half = np.concatenate([gc, cc]), np.concatenate([gh, ch])
    exp = brute_boxes(ctr, half, verts)
    assert (exp["count"][216:] >= 1).all()
    assert_boxes(scene, ctr, half, exp, "after refit")
    scene.destroy()


def test_instanced_scene(ctx):
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
    verts = tri_vertices(pre)
    gc, gh = grid_boxes(*bounds(verts), (8, 6, 6))
    cc, ch = centroid_boxes(verts, every=128)
    ctr, half = np.concatenate([gc, cc]), np.concatenate([gh, ch])
    exp = brute_boxes(ctr, half, verts)
    n1 = c.verts.shape[0]
    assert {int(a[0]) // n1 for a in exp["ids"] if a.size} == {0, 1, 2}
    assert_boxes(scene, ctr, half, exp, "instances")
    scene.destroy()


def test_repeated_device_context_queries_on_the_root(ctx):
    c = case(ctx, "suzanne")
    multi = beam.Context(devices=[0, 0])
    scene, keep = build(multi, c.meshes)
    ctr, half = c.sets["grid"]
    assert_boxes(scene, ctr, half, c.exp["grid"], "devices=[0, 0]")
    scene.destroy()
    multi.close()


# ---- 11. the Python layer ----------------------------------------------------------------------------------
def test_voxelize_equals_the_restated_cells(ctx):
    c = case(ctx, "suzanne")
    lo, hi = bounds(c.verts)
    vox = c.scene.voxelize(lo, hi, (8, 8, 8))
    ctx.sync()  # this context's stream is not torch's
    assert vox.is_cuda and vox.shape == (8, 8, 8) and str(vox.dtype) == "torch.bool"
    want = (c.exp["grid"]["count"] > 0).reshape(8, 8, 8)  # grid_boxes restates the docstring's statements
    assert np.array_equal(vox.cpu().numpy(), want)
    lo2, hi2 = lo - F([0.3, 0.1, 0.7]), hi + F([0.2, 0.9, 0.1])  # cells that are no cubes, dims that differ
    ctr, half = grid_boxes(lo2, hi2, (5, 8, 3))
    vox = c.scene.voxelize(lo2, hi2, (5, 8, 3))
    ctx.sync()
    assert np.array_equal(vox.cpu().numpy(), (brute_boxes(ctr, half, c.verts)["count"] > 0).reshape(5, 8, 3))


def test_torch_chain_into_hit_attributes(ctx):
    """Boxes -> overlapBoxes(mode="list") -> the ids as bm_hit records -> hitAttributes(BM_ATTR_MESH_FACE) on one
    stream: which mesh and face each listed triangle is."""
    import torch
    c = case(ctx, "suzanne")
    dev = torch.device("cuda", 0)
    tctx = beam.Context(device=0, stream=torch.cuda.current_stream(dev).cuda_stream)
    meshes = c.meshes + translated(c.meshes, (0.5, 0.25, -0.5))  # two meshes: the owner is not always mesh 0
    verts = tri_vertices(meshes)
    scene, keep = build(tctx, meshes)
    ctr, half = c.sets["grid"]
    exp = brute_boxes(ctr, half, verts)
    res = scene.overlapBoxes(torch.from_numpy(ctr).to(dev), torch.from_numpy(half).to(dev), mode="list")
    assert res["ids"].is_cuda and res["ids"].dtype == torch.int32 and res["offsets"].shape == (ctr.shape[0] + 1,)
    hits = torch.zeros((res["ids"].shape[0], 4), dtype=torch.float32, device=dev)
    hits.view(torch.int32)[:, 3] = res["ids"]
    (face,) = scene.hitAttributes(hits, [(beam.ATTR_MESH_FACE, 2)])
    packed = torch.zeros((ctr.shape[0], 8), dtype=torch.float32, device=dev)
    packed[:, 0:3], packed[:, 4:7] = torch.from_numpy(ctr).to(dev), torch.from_numpy(half).to(dev)
    hit = scene.overlapBoxes(packed, mode="any")["any"]
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


# ---- 12. errors ----------------------------------------------------------------------------------------------
def test_errors(ctx):
    import torch
    c = case(ctx, "suzanne")
    dev = torch.device("cuda", ctx.device)
    n = 64
    boxes = torch.zeros((n + 1, 8), dtype=torch.float32, device=dev)
    out = torch.zeros((n + 2,), dtype=torch.int32, device=dev)
    off = torch.zeros((n + 2,), dtype=torch.int32, device=dev)
    ids = torch.zeros((64,), dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    bp, op, fp, ip = boxes.data_ptr(), out.data_ptr(), off.data_ptr(), ids.data_ptr()
    unbuilt = beam.IScene.create(ctx)
    assert unbuilt.overlapBoxesDevice(bp, n, COUNT, op) == _lib.ERROR_NOT_BUILT
    unbuilt.destroy()
    s = c.scene
    assert s.overlapBoxesDevice(bp, n, COUNT, op) == 0 and s.overlapBoxesDevice(bp, n, ANY, op) == 0
    assert s.overlapBoxesDevice(bp, n, LIST, op, fp, ip) == 0 and s.overlapBoxesDevice(bp, n, LIST, 0, fp, ip) == 0
    assert s.overlapBoxesDevice(0, 0, COUNT, 0) == 0 and s.overlapBoxesDevice(0, 0, LIST, 0) == 0  # n = 0: nothing read
    for mode in (3, 4, 0x80000000):
        assert s.overlapBoxesDevice(bp, n, mode, op, fp, ip) == BAD
    for flags in (1, 2, 0x80000000):
        assert s.overlapBoxesDevice(bp, n, COUNT, op, flags=flags) == BAD
    assert s.overlapBoxesDevice(0, n, COUNT, op) == BAD and s.overlapBoxesDevice(bp, n, COUNT, 0) == BAD
    assert s.overlapBoxesDevice(bp, n, ANY, 0) == BAD
    assert s.overlapBoxesDevice(bp, n, LIST, op, 0, ip) == BAD and s.overlapBoxesDevice(bp, n, LIST, op, fp, 0) == BAD
    off_b = boxes.view(-1)[1:].data_ptr()            # 4 bytes in
    byte = lambda t: t.view(torch.int8)[1:].data_ptr()  # 1 byte in
    assert off_b == bp + 4 and byte(out) == op + 1
    assert s.overlapBoxesDevice(off_b, n, COUNT, op) == BAD
    assert s.overlapBoxesDevice(boxes.view(-1)[4:].data_ptr(), n, COUNT, op) == 0  # boxes are 16-byte aligned
    assert s.overlapBoxesDevice(bp, n, COUNT, byte(out)) == BAD
    assert s.overlapBoxesDevice(bp, n, ANY, byte(out)) == 0                        # the byte plane: any address
    assert s.overlapBoxesDevice(bp, n, LIST, byte(out), fp, ip) == BAD
    assert s.overlapBoxesDevice(bp, n, LIST, op, byte(off), ip) == BAD
    assert s.overlapBoxesDevice(bp, n, LIST, op, fp, byte(ids)) == BAD
    assert s.overlapBoxesDevice(bp, n, LIST, out[1:].data_ptr(), off[1:].data_ptr(), ids[1:].data_ptr()) == 0
    assert s.overlapBoxesDevice(bp, n, COUNT, op, byte(off), byte(ids)) == 0       # COUNT ignores offsets and ids
    counters = np.zeros(4, np.uint64)
    assert s.overlapBoxesDevice(bp, n, 3, op, counters=counters) == BAD
    assert s.ctx.lib.bm_scene_overlap_boxes_counters(s.h, bp, n, COUNT, 0, op, None, None, None) == BAD
    assert s.ctx.lib.bm_scene_overlap_boxes(None, bp, n, COUNT, 0, op, None, None) == BAD  # a null handle
    ctx.sync()
    with pytest.raises(beam.BeamError):
        s.overlapBoxes(np.zeros((4, 3), F), np.ones((4, 3), F), mode="all")
    tiny = [{"pos": F([[0, 0, 1], [1, 0, 1], [0, 1, 1]]), "nrm": F([[0, 0, 1]] * 3), "idx": np.uint32([0, 1, 2])}]
    # (a BVH8 context exists in A/B builds only: the product library refuses to create one)
    for kw in ({"reference_kd": True}, {"reference_hash": True}, {"bvh_width": 2}):
        other = beam.Context(device=0, **kw)
        sc, keep = build(other, tiny)
        for mode in (COUNT, ANY, LIST):
            assert sc.overlapBoxesDevice(bp, n, mode, op, fp, ip) == BAD, kw
        assert sc.overlapBoxesDevice(bp, n, COUNT, op, counters=counters) == BAD, kw
        sc.destroy()
        other.close()
