"""GPU checks of multi-hit ray queries (bm_scene_trace_rays_multi): the k nearest hits per ray and hit counts.

Every comparison is bit-exact against brute_multi of tests/test_multihit_abi.py: the header's triangle
function restated in numpy float32, evaluated for every triangle and every ray, sorted by (t, id). A
reference is computed once per scene with k = 16 and left unchanged: a smaller k expects its first k columns.
"""
from types import SimpleNamespace

import numpy as np
import pytest

import deep_scenes as ds
from raytracercuda_amd import _lib, beam, scenes
from test_multihit_abi import (F, LAYERS, NO_TRI, bits, brute_multi, layers_mesh, layers_rays, make_batch, tiny_scene,
                               tri_vertices)

pytestmark = pytest.mark.gpu

ALL = _lib.MULTI_COUNT_ALL
BAD = _lib.ERROR_INVALID_PARAMETER
KMAX = _lib.MULTI_MAX_HITS
KEYS = ("t", "u", "v", "tri_id")


def build(ctx, meshes):
    scene = beam.IScene.create(ctx)
    keep = beam.upload_meshes(ctx, scene, meshes)
    scene.updateGPUScene()
    return scene, keep


def frozen(res):
    for a in res.values():
        a.setflags(write=False)
    return res


_CASES = {}


def replicated(single, copies, n1, k=KMAX):
    """brute_multi's answer for a mesh added `copies` times (ids g, g + N, ...), from its answer `single` for the
    mesh alone, all of whose hits fit its columns: the copies are bit-equal, so each hit becomes `copies`
    records of one t, u, v in id order. Checked against brute_multi itself on the tripled scene."""
    assert int(single["count"].max()) <= single["t"].shape[1]
    out = {key: np.repeat(single[key], copies, axis=1)[:, :k] for key in ("t", "u", "v")}
    ids = np.repeat(single["tri_id"].astype(np.int64), copies, axis=1)
    ids = np.where(ids == NO_TRI, NO_TRI, ids + np.tile(np.arange(copies) * n1, single["t"].shape[1])[None, :])
    out["tri_id"] = ids[:, :k].astype(np.uint32)
    out["count"] = single["count"] * np.uint32(copies)
    return out


def case(ctx, name):
    """Meshes, GPU scene, rays and brute_multi's k = 16 answer — made once per module run."""
    if name not in _CASES:
        copies = {"suzanne3": 3, "suzanne6": 6}.get(name, 1)  # ids g, g + N, ...: bit-equal t
        if name == "layers":
            meshes = layers_mesh()
            o, d = layers_rays()
        else:
            one = scenes.load_mesh("suzanne" if copies > 1 else name)
            meshes = one * copies
            o, d = make_batch(one)
        verts = tri_vertices(meshes)
        scene, keep = build(ctx, meshes)
        if name == "suzanne6":  # 91 million pairs: from the single mesh's answer instead
            exp = replicated(case(ctx, "suzanne").exp, 6, verts.shape[0] // 6)
        else:
            exp = brute_multi(o, d, np.inf, verts, KMAX)
        _CASES[name] = SimpleNamespace(meshes=meshes, verts=verts, scene=scene, keep=keep, o=o, d=d, exp=frozen(exp))
    return _CASES[name]


def teardown_module(module):
    for k in _CASES.values():
        k.scene.destroy()
    _CASES.clear()


def assert_multi(res, exp, k, count_all=False, where=None):
    """res (k records per ray) equals the first k columns of exp (brute_multi with at least k), counts included."""
    sel = slice(None) if where is None else where
    assert res["tri_id"].shape[1] == k
    assert np.array_equal(res["tri_id"][sel], exp["tri_id"][sel][:, :k]), \
        f"tri_id differs on {int((res['tri_id'][sel] != exp['tri_id'][sel][:, :k]).any(axis=1).sum())} rays"
    for key in ("t", "u", "v"):
        assert np.array_equal(bits(res[key][sel]), bits(exp[key][sel][:, :k])), key
    want = exp["count"][sel] if count_all else np.minimum(exp["count"][sel], k)
    assert np.array_equal(res["count"][sel], want), "count"


# ---- 1. layers: the list fills and the traversal keeps going -------------------------------------------
@pytest.mark.parametrize("count_all", [False, True])
@pytest.mark.parametrize("k", [1, 2, 3, 4, 5, 8, 15, 16])
def test_layers(ctx, k, count_all):
    c = case(ctx, "layers")
    assert c.verts.shape[0] == 432 and c.o.shape[0] == 500
    assert float((c.exp["count"] > 16).mean()) == 1.0  # every ray fills the longest list and has more behind it
    assert np.all(c.exp["count"] == LAYERS)
    res = c.scene.traceRaysMulti(c.o, c.d, k=k, count_all=count_all)
    assert_multi(res, c.exp, k, count_all)
    assert np.all(res["count"] == (LAYERS if count_all else k))
    assert np.all(res["tri_id"] != NO_TRI)


def test_layers_tmax_at_and_below_the_seventh_hit(ctx):
    c = case(ctx, "layers")
    t7 = np.ascontiguousarray(c.exp["t"][:, 6])
    for tmax, crossings in ((t7, 7), (np.nextafter(t7, F(0.0)), 6)):
        exp = brute_multi(c.o, c.d, tmax, c.verts, KMAX)
        assert np.all(exp["count"] == crossings)
        for k in (4, 8, 16):
            for count_all in (False, True):
                res = c.scene.traceRaysMulti(c.o, c.d, tmax=tmax, k=k, count_all=count_all)
                assert_multi(res, exp, k, count_all)


def test_layers_pure_count_writes_only_counts(ctx):
    import torch
    c = case(ctx, "layers")
    dev = torch.device("cuda", ctx.device)
    n = c.o.shape[0]
    packed = np.zeros((n, 8), F)
    packed[:, 0:3], packed[:, 3], packed[:, 4:7] = c.o, np.inf, c.d
    rays = torch.from_numpy(packed).to(dev)
    counts = torch.full((n + 64,), -3, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    assert c.scene.traceRaysMultiDevice(rays.data_ptr(), n, 0, 0, counts.data_ptr(), ALL) == 0
    ctx.sync()
    got = counts.cpu().numpy()
    assert np.all(got[:n] == LAYERS) and np.all(got[n:] == -3)
    res = c.scene.traceRaysMulti(c.o, c.d, k=0, count_all=True)  # the wrapper's k = 0
    assert res["t"].shape == (n, 0) and np.all(res["count"] == LAYERS)


# ---- 2. ties at the list's edge ------------------------------------------------------------------------
# Suzanne added three times: |H| in {0, 6, 9, ..., 24}, ties only in triples, k = 4 and k = 5 cut through one.
# Of its 976 rays only 5 (0.5 %) have |H| > 16: 58 rays cross the single mesh three times or more and 8 times at
# most, so a tripled scene cannot reach the 5 % this test asks for k = 16's edge. Suzanne added six times does
# (every ray with three crossings or more has 18: 5.9 %), with ties in sixes that k = 4, 5 and 16 all cut
# through; the assertion is made there and both scenes run.
@pytest.mark.parametrize("k", [1, 2, 4, 5, 16])
@pytest.mark.parametrize("name", ["suzanne3", "suzanne6"])
def test_ties_resolve_to_the_lowest_ids(ctx, name, k):
    c = case(ctx, name)
    copies = int(name[-1])
    n1 = c.verts.shape[0] // copies
    cnt = c.exp["count"]
    assert 0.1 <= float((cnt > 0).mean()) <= 0.9
    deep = float((cnt > 16).mean())
    print(f"{name}: {deep:.3f} of the rays have |H| > 16")
    assert deep >= 0.05 if copies == 6 else deep > 0.0, deep
    assert np.all(cnt % copies == 0) and int(cnt.max()) == 8 * copies and int(cnt[cnt > 0].min()) == 2 * copies
    hit = np.flatnonzero(cnt > 0)
    e = c.exp
    # the reference itself: groups g, g + N, ... with one t; k = 4 and k = 5 cut through the second (first) group
    for j in range(1, copies):
        assert np.array_equal(e["tri_id"][hit, j], e["tri_id"][hit, 0] + j * n1)
        assert np.array_equal(bits(e["t"][hit, j]), bits(e["t"][hit, 0]))
    assert np.all(e["t"][hit, copies] > e["t"][hit, copies - 1])
    if copies == 3:
        assert np.array_equal(e["tri_id"][hit, 4], e["tri_id"][hit, 3] + n1)
        # the short cut the six-fold scene's reference takes, against the brute force on this one
        rep = replicated(case(ctx, "suzanne").exp, 3, n1)
        for key in KEYS + ("count",):
            assert np.array_equal(rep[key].view(np.uint32), e[key].view(np.uint32)), key
    for count_all in (False, True):
        res = c.scene.traceRaysMulti(c.o, c.d, k=k, count_all=count_all)
        assert_multi(res, c.exp, k, count_all)


# ---- 3. meshes -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [1, 4, 16])
@pytest.mark.parametrize("name", ["suzanne", "bunny"])
def test_meshes(ctx, name, k):
    c = case(ctx, name)
    assert c.o.shape[0] == 976
    assert 0.1 <= float((c.exp["count"] > 0).mean()) <= 0.9
    assert_multi(c.scene.traceRaysMulti(c.o, c.d, k=k), c.exp, k)
    assert_multi(c.scene.traceRaysMulti(c.o, c.d, k=k, count_all=True), c.exp, k, True)


# ---- 4. agreement with the closest query ---------------------------------------------------------------
def agreement(scene, o, d, exp=None):
    """The invariants between the multi-hit query at k = 1, 4, 16 and the closest query on the same rays."""
    closest = scene.traceRays(o, d, counters=True)
    r1 = scene.traceRaysMulti(o, d, k=1, counters=True)
    r4 = scene.traceRaysMulti(o, d, k=4, counters=True)
    r16 = scene.traceRaysMulti(o, d, k=16, counters=True)
    a16 = scene.traceRaysMulti(o, d, k=16, count_all=True, counters=True)
    for r in (r1, r4, r16, a16):  # record 0 is the closest query's record, bit for bit
        assert np.array_equal(r["tri_id"][:, 0], closest["tri_id"])
        for key in ("t", "u", "v"):
            assert np.array_equal(bits(r[key][:, 0]), bits(closest[key])), key
    for key in KEYS:  # k = 4's records are the first four of k = 16's; counting all changes no record
        assert np.array_equal(r4[key].view(np.uint32), r16[key].view(np.uint32)[:, :4]), key
        assert np.array_equal(r16[key].view(np.uint32), a16[key].view(np.uint32)), key
    # k = 1 without the flag is quad_closest's sequence of visits and leaf tests
    assert int(r1["counters"][0]) == int(closest["counters"][0]) and int(r1["counters"][1]) == int(closest["counters"][1])
    assert int(r1["counters"][2]) == int(closest["counters"][2]) == int((closest["tri_id"] != NO_TRI).sum())
    assert int(r16["counters"][0]) >= int(r4["counters"][0]) >= int(r1["counters"][0])
    assert int(a16["counters"][0]) >= int(r16["counters"][0]) and int(a16["counters"][1]) >= int(r16["counters"][1])
    assert int(r16["counters"][2]) == int(r16["count"].sum()) and int(a16["counters"][2]) == int(a16["count"].sum())
    assert np.all(a16["count"] >= r16["count"])
    if exp is not None:
        assert_multi(r4, exp, 4)
    return r4


@pytest.mark.parametrize("name", ["layers", "suzanne3", "suzanne6", "suzanne", "bunny"])
def test_agreement_with_the_closest_query(ctx, name):
    c = case(ctx, name)
    agreement(c.scene, c.o, c.d, c.exp)


# ---- 5. stack overflow ---------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["deep", "deep+dup-leaf1"])
def test_deep_scenes_use_the_overflow_area(name):
    _, dup, leaf = ds.scene_of(name)
    dctx = beam.Context(device=0, leaf_size=leaf)
    meshes = ds.deep_meshes(dup)
    scene, keep = build(dctx, meshes)
    o, d = ds.ray_batch()
    verts = tri_vertices(meshes)
    assert o.shape[0] * verts.shape[0] < 5e7  # every ray against every triangle
    exp = brute_multi(o, d, np.inf, verts, KMAX)
    assert (exp["count"] > 0).any()
    r4 = agreement(scene, o, d, exp)  # k = 1 equals the closest query: its traversal, so the overflow side runs
    assert_multi(r4, exp, 4)
    assert_multi(scene.traceRaysMulti(o, d, k=16, count_all=True), exp, 16, True)
    scene.destroy()
    dctx.close()


# ---- 6. edges ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [0, 1, 3, 15, 16, 17, 63, 64, 65, 1025])
def test_batch_edges_write_nothing_past_n(ctx, n):
    import torch
    c = case(ctx, "suzanne3")
    dev = torch.device("cuda", ctx.device)
    idx = np.arange(n) % c.o.shape[0]
    rays = np.zeros((max(n, 1), 8), F)
    rays[:n, 0:3], rays[:n, 3], rays[:n, 4:7] = c.o[idx], np.inf, c.d[idx]
    r_dev = torch.from_numpy(rays).to(dev)
    for k in (3, 16):
        hits = torch.full((n * k + 64, 4), -7.5, dtype=torch.float32, device=dev)
        counts = torch.full((n + 64,), -3, dtype=torch.int32, device=dev)
        torch.cuda.synchronize()
        assert c.scene.traceRaysMultiDevice(r_dev.data_ptr(), n, k, hits.data_ptr(), counts.data_ptr()) == 0
        ctx.sync()
        h, cn = hits.cpu().numpy(), counts.cpu().numpy()
        assert np.all(h[n * k:] == F(-7.5)) and np.all(cn[n:] == -3)
        h = h[:n * k].reshape(n, k, 4)
        got = {"t": h[..., 0], "u": h[..., 1], "v": h[..., 2], "tri_id": h.view(np.uint32)[..., 3],
               "count": cn[:n].view(np.uint32)}
        assert_multi(got, {key: val[idx] for key, val in c.exp.items()}, k)


def test_small_grid_strides_over_the_batches(ctx):
    c = case(ctx, "suzanne3")
    small = beam.Context(device=0, params={"trace_grid": 2})  # 8 waves: several batches each
    scene, keep = build(small, c.meshes)
    for k in (4, 16):
        assert_multi(scene.traceRaysMulti(c.o, c.d, k=k), c.exp, k)
    assert_multi(scene.traceRaysMulti(c.o, c.d, k=16, count_all=True), c.exp, 16, True)
    scene.destroy()
    small.close()


def test_empty_built_scene(ctx):
    c = case(ctx, "suzanne")
    scene, keep = build(ctx, [])
    for k, count_all in ((1, False), (16, False), (4, True), (0, True)):
        res = scene.traceRaysMulti(c.o[:100], c.d[:100], k=k, count_all=count_all, counters=True)
        assert np.all(res["tri_id"] == NO_TRI) and np.all(np.isposinf(res["t"])) and np.all(res["count"] == 0)
        assert np.all(bits(res["u"]) == 0) and np.all(bits(res["v"]) == 0)
        assert int(res["counters"][1]) == 0 and int(res["counters"][2]) == 0
    scene.destroy()


@pytest.mark.parametrize("ntri", [1, 2, 5, 17])
def test_tiny_scenes(ctx, ntri):
    meshes, eyes, o, d = tiny_scene(ntri)
    scene, keep = build(ctx, meshes)
    exp = brute_multi(o, d, np.inf, tri_vertices(meshes), KMAX)
    agreement(scene, o, d, exp)
    for k in (1, 2, 5, 16):
        assert_multi(scene.traceRaysMulti(o, d, k=k), exp, k)
        assert_multi(scene.traceRaysMulti(o, d, k=k, count_all=True), exp, k, True)
    scene.destroy()


def test_axis_parallel_and_invalid_rays(ctx):
    """The table of tests/test_gpu_rays.py test 7 on every seventh ray."""
    c = case(ctx, "suzanne")
    n = c.o.shape[0]
    o, d = c.o.copy(), c.d.copy()
    tmax = np.full(n, np.inf, F)
    sel = np.arange(0, n, 7)
    kind = (sel // 7) % 7
    d[sel[kind == 0], 1] = 0.0           # one zero component
    d[sel[kind == 1], 0] = 0.0           # two
    d[sel[kind == 1], 2] = 0.0
    o[sel[kind == 2], 1] = np.nan
    d[sel[kind == 3], 2] = np.inf
    tmax[sel[kind == 4]] = np.nan
    tmax[sel[kind == 5]] = 0.0
    tmax[sel[kind == 6]] = -1.0
    invalid = np.zeros(n, bool)
    invalid[sel[kind >= 2]] = True
    exp = brute_multi(o, d, tmax, c.verts, KMAX)
    assert np.all(exp["count"][invalid] == 0) and (exp["count"][sel[kind <= 1]] > 0).any()
    valid_only = brute_multi(o[~invalid], d[~invalid], tmax[~invalid], c.verts, 1)
    for k, count_all in ((1, False), (5, False), (16, False), (16, True)):
        res = c.scene.traceRaysMulti(o, d, tmax=tmax, k=k, count_all=count_all, counters=True)
        assert_multi(res, exp, k, count_all)
        assert np.all(res["tri_id"][invalid] == NO_TRI) and np.all(np.isposinf(res["t"][invalid]))
        assert np.all(bits(res["u"][invalid]) == 0) and np.all(bits(res["v"][invalid]) == 0)
        assert np.all(res["count"][invalid] == 0)
        if k == 1:  # invalid rays count nothing: the counters are those of the valid rays alone
            alone = c.scene.traceRaysMulti(o[~invalid], d[~invalid], tmax=tmax[~invalid], k=1, counters=True)
            assert_multi(alone, valid_only, 1)
            assert list(map(int, res["counters"])) == list(map(int, alone["counters"]))


def test_query_after_refit(ctx):
    c = case(ctx, "bunny")
    scene = beam.IScene.create(ctx)
    meshes = beam.upload_meshes(ctx, scene, c.meshes)
    scene.updateGPUScene()
    moved = []
    for m in c.meshes:
        p = np.asarray(m["pos"], F)
        q = p.copy()
        q[:, 1] += F(0.03) * np.sin(F(8.0) * p[:, 0] + F(1.0)).astype(F)
        q[:, 0] += F(0.009) * np.cos(F(5.0) * p[:, 2]).astype(F)
        moved.append(dict(m, pos=q))
    for m, mv in zip(meshes, moved):
        assert m.setVertexData(mv["pos"], mv["pos"].shape[0], 3, beam.VERTEX_DATA_POSITION) == 0
    scene.refitGPUScene()
    n = 4 * 61
    exp = brute_multi(c.o[:n], c.d[:n], np.inf, tri_vertices(moved), KMAX)
    assert (exp["count"] > 0).any() and not np.array_equal(exp["tri_id"], c.exp["tri_id"][:n])
    for k in (4, 16):
        assert_multi(scene.traceRaysMulti(c.o[:n], c.d[:n], k=k, count_all=True), exp, k, True)
    scene.destroy()


def test_rehearsal_context_queries_on_the_root(ctx):
    c = case(ctx, "suzanne3")
    multi = beam.Context(devices=[0, 0])
    scene, keep = build(multi, c.meshes)
    assert_multi(scene.traceRaysMulti(c.o, c.d, k=5), c.exp, 5)
    assert_multi(scene.traceRaysMulti(c.o, c.d, k=16, count_all=True), c.exp, 16, True)
    scene.destroy()
    multi.close()


# ---- 7. errors -----------------------------------------------------------------------------------------
def test_errors(ctx):
    import torch
    c = case(ctx, "suzanne")
    dev = torch.device("cuda", ctx.device)
    n = 64
    rays = torch.zeros((n + 1, 8), dtype=torch.float32, device=dev)
    out = torch.zeros((n * 16 + 1, 4), dtype=torch.float32, device=dev)
    cnt = torch.zeros((n + 1,), dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    rp, op, cp = rays.data_ptr(), out.data_ptr(), cnt.data_ptr()
    unbuilt = beam.IScene.create(ctx)
    assert unbuilt.traceRaysMultiDevice(rp, n, 4, op, cp) == _lib.ERROR_NOT_BUILT
    unbuilt.destroy()
    s = c.scene
    assert s.traceRaysMultiDevice(rp, n, 4, op) == 0 and s.traceRaysMultiDevice(rp, n, 16, op, cp, ALL) == 0
    assert s.traceRaysMultiDevice(rp, n, 0, 0, cp, ALL) == 0          # a pure count needs no hit records
    assert s.traceRaysMultiDevice(0, 0, 4, 0) == 0                    # n = 0: nothing to read or write
    assert s.traceRaysMultiDevice(rp, n, 0, op, cp) == BAD            # k = 0 without the flag
    assert s.traceRaysMultiDevice(rp, n, 17, op, cp) == BAD
    assert s.traceRaysMultiDevice(rp, n, 17, op, cp, ALL) == BAD
    for flags in (2, 3, 0x80000000):
        assert s.traceRaysMultiDevice(rp, n, 4, op, cp, flags) == BAD
    assert s.traceRaysMultiDevice(0, n, 4, op, cp) == BAD and s.traceRaysMultiDevice(rp, n, 4, 0, cp) == BAD
    assert s.traceRaysMultiDevice(rp, n, 4, op, 0, ALL) == BAD        # null counts with the flag
    off_r, off_o = rays.view(-1)[1:].data_ptr(), out.view(-1)[1:].data_ptr()  # 4 bytes in
    off_c = cnt.view(torch.int8)[1:].data_ptr()                              # 1 byte in
    assert off_r == rp + 4 and off_o == op + 4 and off_c == cp + 1
    assert s.traceRaysMultiDevice(off_r, n, 4, op, cp) == BAD and s.traceRaysMultiDevice(rp, n, 4, off_o, cp) == BAD
    assert s.traceRaysMultiDevice(rp, n, 4, op, off_c) == BAD
    assert s.traceRaysMultiDevice(rp, n, 4, op, cnt[1:].data_ptr()) == 0  # counts are 4-byte aligned
    counters = np.zeros(3, np.uint64)
    assert s.traceRaysMultiDevice(rp, n, 17, op, cp, 0, counters) == BAD
    ctx.sync()
    tiny = [{"pos": F([[0, 0, 1], [1, 0, 1], [0, 1, 1]]), "nrm": F([[0, 0, 1]] * 3), "idx": np.uint32([0, 1, 2])}]
    for kw in ({"reference_kd": True}, {"reference_hash": True}, {"bvh_width": 2}):
        other = beam.Context(device=0, **kw)
        sc, keep = build(other, tiny)
        assert sc.traceRaysMultiDevice(rp, n, 4, op, cp) == BAD, kw
        assert sc.traceRaysMultiDevice(rp, n, 4, op, cp, ALL) == BAD, kw
        sc.destroy()
        other.close()


# ---- 8. torch ------------------------------------------------------------------------------------------
def test_torch_chain_stays_on_the_device():
    """Packed rays -> traceRaysMulti(k=4) -> hitAttributes(position) on one stream without a wait. The positions
    are compared bit for bit with tests/test_gpu_attrs.py's restatement of the interpolation (its tolerance
    for these rows: none) and with o + d*t. For the latter: t, u and v each come out of a dozen float32
    roundings on magnitudes up to S = |o| + |d| t + max |vertex|, divided by det = |d| |e1 x e2| cos(angle to
    the normal), so the interpolated point and o + d*t differ by a few dozen units of 2^-24 S / cos; the bound
    is 256 of them, over the hits with cos >= 0.05."""
    import torch
    from test_gpu_attrs import expected
    meshes = scenes.load_mesh("suzanne")
    o, d = make_batch(meshes)
    dev = torch.device("cuda", 0)
    tctx = beam.Context(device=0, stream=torch.cuda.current_stream(dev).cuda_stream)
    scene, keep = build(tctx, meshes)
    n, k = o.shape[0], 4
    packed = np.zeros((n, 8), F)
    packed[:, 0:3], packed[:, 3], packed[:, 4:7] = o, np.inf, d
    rays = torch.from_numpy(packed).to(dev)
    # no synchronisation from here to the end of the chain
    res = scene.traceRaysMulti(rays, k=k)
    assert res["hits"].is_cuda and res["hits"].shape == (n, k, 4) and res["tri_id"].dtype == torch.int32
    assert res["t"].shape == (n, k) and res["count"].shape == (n,) and res["count"].dtype == torch.int32
    (pos,) = scene.hitAttributes(res["hits"].view(-1, 4), [(beam.VERTEX_DATA_POSITION, 3)])
    assert pos.is_cuda and pos.shape == (n * k, 3)
    along = (rays[:, None, 0:3] + rays[:, None, 4:7] * res["t"][:, :, None]).reshape(-1, 3)
    torch.cuda.synchronize()
    verts = tri_vertices(meshes)
    exp = brute_multi(o, d, np.inf, verts, k)
    hits = res["hits"].cpu().numpy()
    got = {"t": hits[..., 0], "u": hits[..., 1], "v": hits[..., 2], "tri_id": hits.view(np.uint32)[..., 3],
           "count": res["count"].cpu().numpy().view(np.uint32)}
    assert_multi(got, exp, k)
    p = pos.cpu().numpy()
    flat = hits.reshape(-1, 4)
    want = expected(meshes, flat, beam.VERTEX_DATA_POSITION, 3)
    assert np.array_equal(p.view(np.uint32), want.view(np.uint32))
    filled = flat.view(np.uint32)[:, 3] != NO_TRI
    assert np.all(p[~filled].view(np.uint32) == 0) and 0 < int(filled.sum()) < n * k  # miss slots: zero rows
    g = flat.view(np.uint32)[filled, 3]
    v64 = verts[g].astype(np.float64)
    nrm = np.cross(v64[:, 1] - v64[:, 0], v64[:, 2] - v64[:, 0])
    dd = np.repeat(d, k, axis=0)[filled].astype(np.float64)
    oo = np.repeat(o, k, axis=0)[filled].astype(np.float64)
    cos = np.abs((nrm * dd).sum(1)) / (np.linalg.norm(nrm, axis=1) * np.linalg.norm(dd, axis=1))
    scale = np.abs(oo).max(1) + np.abs(dd).max(1) * flat[filled, 0] + np.abs(v64).max(axis=(1, 2))
    err = np.abs(p[filled].astype(np.float64) - along.cpu().numpy()[filled]).max(1)
    steep = cos >= 0.05
    assert steep.sum() > 100
    ratio = err[steep] / (2.0 ** -24 * scale[steep] / cos[steep])
    print(f"torch chain: largest |position - (o + d t)| = {ratio.max():.1f} units of 2^-24 S / cos")
    assert ratio.max() <= 256.0
    scene.destroy()
    tctx.close()
