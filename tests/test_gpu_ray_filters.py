"""GPU checks of the ray query filters: tmin, skip-triangle, face culling and entry masks in
bm_scene_trace_rays (closest, any hit) and bm_scene_trace_rays_multi.

Every comparison is bit for bit against brute_filtered of tests/test_ray_filters_abi.py: the header's triangle
function and filter restated in numpy float32, evaluated for every triangle and every ray. A reference is computed
once per (scene, filter) with k = 16 and left unchanged: a smaller k expects its first k columns, the closest
query its first column.
"""
import ctypes as C
from types import SimpleNamespace

import numpy as np
import pytest

import deep_scenes as ds
from raytracercuda_amd import _lib, beam, scenes
from test_gpu_instances import frame
from test_gpu_multihit import assert_multi, build, frozen
from test_instances_abi import xform_mesh
from test_multihit_abi import F, NO_TRI, bits, make_batch, tiny_scene, tri_vertices
from test_ray_filters_abi import ALL_ONES, BACK, FRONT, MASK, SKIP, TMIN, brute_filtered, fixture

pytestmark = pytest.mark.gpu

ALL = _lib.MULTI_COUNT_ALL
BAD = _lib.ERROR_INVALID_PARAMETER
KMAX = _lib.MULTI_MAX_HITS
CULLS = {"back": BACK, "front": FRONT}

_CASES = {}


def case(ctx, name):
    """Meshes, vertices, GPU scene and rays of a facing fixture, made once per module run."""
    if name not in _CASES:
        meshes, verts, o, d = fixture(name)
        scene, keep = build(ctx, meshes)
        _CASES[name] = SimpleNamespace(meshes=meshes, verts=verts, scene=scene, keep=keep, o=o, d=d, exp={})
    return _CASES[name]


def expect(c, flags=0, pad=0, tmax=np.inf, scale=1.0):
    """brute_filtered's k = 16 answer for the case's rays (directions scaled by `scale`), cached for scalar pads."""
    key = (flags, pad, scale) if np.isscalar(pad) and np.isscalar(tmax) and np.isinf(tmax) else None
    if key is None or key not in c.exp:
        e = frozen(brute_filtered(c.o, c.d * F(scale), tmax, pad, flags, c.verts, k=KMAX))
        if key is None:
            return e
        c.exp[key] = e
    return c.exp[key]


def teardown_module(module):
    for k in _CASES.values():
        k.scene.destroy()
    _CASES.clear()


def assert_closest(res, exp, where=None):
    sel = slice(None) if where is None else where
    assert np.array_equal(res["tri_id"][sel], exp["tri_id"][sel, 0]), \
        f"tri_id differs on {int((res['tri_id'][sel] != exp['tri_id'][sel, 0]).sum())} rays"
    for key in ("t", "u", "v"):
        assert np.array_equal(bits(res[key][sel]), bits(exp[key][sel, 0])), key


def check_all_modes(scene, o, d, exp, any_exp=None, scale=1.0, tmax=None, **kw):
    """Closest, any hit (on directions scaled by `scale`, against any_exp), multi k = 4 and count-all k = 16."""
    assert_closest(scene.traceRays(o, d, tmax=tmax, **kw), exp)
    any_exp = exp if any_exp is None else any_exp
    occ = scene.traceRays(o, d * F(scale), any_hit=True, **kw)["occluded"]
    assert np.array_equal(occ, any_exp["occluded"]), f"occluded differs on {int((occ != any_exp['occluded']).sum())} rays"
    assert_multi(scene.traceRaysMulti(o, d, tmax=tmax, k=4, **kw), exp, 4)
    assert_multi(scene.traceRaysMulti(o, d, tmax=tmax, k=16, count_all=True, **kw), exp, 16, True)


def same_as_unflagged(scene, o, d, d_any, **kw):
    """Results and all counters of a filter that can reject nothing equal those of flags = 0, bit for bit."""
    for any_hit in (False, True):
        dd = d_any if any_hit else d
        a = scene.traceRays(o, dd, any_hit=any_hit, counters=True)
        b = scene.traceRays(o, dd, any_hit=any_hit, counters=True, **kw)
        for key in a:
            assert np.array_equal(a[key].view(np.uint8), b[key].view(np.uint8)), (any_hit, key)
    for k, count_all in ((1, False), (4, False), (16, False), (16, True), (0, True)):
        a = scene.traceRaysMulti(o, d, k=k, count_all=count_all, counters=True)
        b = scene.traceRaysMulti(o, d, k=k, count_all=count_all, counters=True, **kw)
        for key in a:
            assert np.array_equal(a[key].view(np.uint8), b[key].view(np.uint8)), (k, count_all, key)


# ---- 1. facing -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["layers", "suzanne"])
def test_facing(ctx, name):
    c = case(ctx, name)
    assert (c.verts.shape[0], c.o.shape[0]) == (432, 500) if name == "layers" else c.o.shape[0] == 976
    scale = 0.3 if name == "layers" else 1.0  # any hit: segments that end inside the stack
    counts = {}
    for cull, flag in CULLS.items():
        exp, any_exp = expect(c, flag), expect(c, flag, scale=scale)
        assert exp["count"].sum() > 0 and 0 < any_exp["occluded"].sum()
        assert_closest(c.scene.traceRays(c.o, c.d, cull=cull), exp)
        occ = c.scene.traceRays(c.o, c.d * F(scale), any_hit=True, cull=cull)["occluded"]
        assert np.array_equal(occ, any_exp["occluded"])
        for k in (4, 16):
            assert_multi(c.scene.traceRaysMulti(c.o, c.d, k=k, cull=cull), exp, k)
        for k in (0, 16):
            res = c.scene.traceRaysMulti(c.o, c.d, k=k, count_all=True, cull=cull)
            assert_multi(res, exp, k, True)
        counts[cull] = res["count"]
    both = c.scene.traceRaysMulti(c.o, c.d, k=0, count_all=True)["count"]
    assert np.array_equal(counts["back"] + counts["front"], both)
    assert not np.array_equal(expect(c, BACK)["tri_id"], expect(c, FRONT)["tri_id"])
    if name == "layers":  # reversed odd layers: half of the 24 crossings face each way
        assert np.all(counts["back"] == 12) and np.all(counts["front"] == 12)


def test_facing_of_a_mirrored_instance(ctx):
    """Facing is the world-space triangle's: a mirroring matrix flips it, as it flips BM_ATTR_GEOM_NORMAL."""
    suz = scenes.load_mesh("suzanne")
    mirror = F([[-1, 0, 0, 0], [0, 1, 0, 0], [0, 0, 1, 0]])
    scene = beam.IScene.create(ctx)
    meshes = beam.upload_meshes(ctx, scene, suz)
    for m in meshes:
        scene.removeMesh(m)
        scene.addInstance(m, mirror)
    scene.updateGPUScene()
    world = [xform_mesh(mirror, m) for m in suz]
    verts = tri_vertices(world)
    o, d = make_batch(world)
    plain = brute_filtered(o, d, np.inf, 0, BACK, tri_vertices(suz), k=4)
    for cull, flag in CULLS.items():
        exp = brute_filtered(o, d, np.inf, 0, flag, verts, k=4)
        assert_multi(scene.traceRaysMulti(o, d, k=4, cull=cull), exp, 4)
    # mirrored rays against the mirrored mesh see the faces the other way round
    om, dm = o * F([-1, 1, 1]), d * F([-1, 1, 1])
    flipped = brute_filtered(om, dm, np.inf, 0, FRONT, tri_vertices(suz), k=4)
    got = scene.traceRaysMulti(o, d, k=4, cull="back")
    assert np.array_equal(got["tri_id"], brute_filtered(o, d, np.inf, 0, BACK, verts, k=4)["tri_id"])
    assert np.array_equal(got["tri_id"], flipped["tri_id"]) and not np.array_equal(got["tri_id"], plain["tri_id"])
    scene.destroy()


# ---- 2. skip -------------------------------------------------------------------------------------------
def test_skip_cures_self_intersection(ctx):
    c = case(ctx, "suzanne")
    first = expect(c)
    hit = np.flatnonzero(first["count"] > 0)
    assert hit.size > 200
    rng = np.random.default_rng(41)
    o2 = (c.o[hit] + c.d[hit] * first["t"][hit, :1]).astype(F)  # float32: on the surface to rounding
    d2 = F(rng.normal(size=(hit.size, 3)))
    ids = first["tri_id"][hit, 0]
    exp = brute_filtered(o2, d2, np.inf, ids, SKIP, c.verts, k=KMAX)
    assert not (exp["tri_id"] == ids[:, None]).any()
    check_all_modes(c.scene, o2, d2, exp, skip_tri=ids)
    plain = c.scene.traceRays(o2, d2)
    again = int((plain["tri_id"] == ids).sum())
    print(f"skip: {again} of {hit.size} unflagged second rays hit the triangle they start on; "
          f"{int((plain['tri_id'] != exp['tri_id'][:, 0]).sum())} differ from the skipping query")


def test_skip_returns_the_twin_of_a_mesh_added_twice(ctx):
    c = case(ctx, "suzanne")
    ntri = c.verts.shape[0]
    scene, keep = build(ctx, c.meshes * 2)
    first = scene.traceRays(c.o, c.d)
    hit = first["tri_id"] != NO_TRI
    assert hit.sum() > 200 and np.all(first["tri_id"][hit] < ntri)
    res = scene.traceRays(c.o, c.d, skip_tri=first["tri_id"])
    assert np.array_equal(res["tri_id"][hit], first["tri_id"][hit] + ntri)
    assert np.array_equal(res["tri_id"][~hit], first["tri_id"][~hit])
    for key in ("t", "u", "v"):
        assert np.array_equal(bits(res[key]), bits(first[key])), key
    verts2 = np.concatenate([c.verts, c.verts])
    exp = brute_filtered(c.o, c.d, np.inf, first["tri_id"], SKIP, verts2, k=KMAX)
    check_all_modes(scene, c.o, c.d, exp, skip_tri=first["tri_id"])
    scene.destroy()


def test_skip_of_no_triangle_equals_unflagged(ctx):
    c = case(ctx, "suzanne")
    for pad in (NO_TRI, c.verts.shape[0] + 5):
        same_as_unflagged(c.scene, c.o, c.d, c.d, skip_tri=pad)
    same_as_unflagged(c.scene, c.o, c.d, c.d, skip_tri=-1)


# ---- 3. tmin -------------------------------------------------------------------------------------------
def test_tmin_is_strict(ctx):
    c = case(ctx, "layers")
    multi = c.scene.traceRaysMulti(c.o, c.d, k=16)
    assert_multi(multi, expect(c), 16)
    t7 = np.ascontiguousarray(multi["t"][:, 6])
    for tmin, col in ((t7, 7), (np.nextafter(t7, F(0.0)), 6)):
        exp = expect(c, TMIN, bits(tmin))
        assert np.array_equal(exp["tri_id"][:, 0], multi["tri_id"][:, col]) and np.all(exp["count"] == 24 - col)
        res = c.scene.traceRays(c.o, c.d, tmin=tmin)
        assert_closest(res, exp)
        assert np.array_equal(bits(res["t"]), bits(multi["t"][:, col]))
        check_all_modes(c.scene, c.o, c.d, exp, tmin=tmin)
    # with both bounds: t7 < t <= tmax
    t10 = np.ascontiguousarray(multi["t"][:, 9])
    exp = expect(c, TMIN, bits(t7), tmax=t10)
    assert np.all(exp["count"] == 3)
    assert_multi(c.scene.traceRaysMulti(c.o, c.d, tmax=t10, k=4, count_all=True, tmin=t7), exp, 4, True)
    assert_multi(c.scene.traceRaysMulti(c.o, c.d, tmax=t10, k=2, tmin=t7), exp, 2)


def test_tmin_zero_equals_unflagged(ctx):
    for name in ("layers", "suzanne"):
        c = case(ctx, name)
        same_as_unflagged(c.scene, c.o, c.d, c.d * F(0.3), tmin=0.0)


def test_tmin_at_or_beyond_tmax_misses(ctx):
    c = case(ctx, "layers")
    t7 = np.ascontiguousarray(expect(c)["t"][:, 6])
    for tmin in (t7, t7 * F(2.0)):
        res = c.scene.traceRays(c.o, c.d, tmax=t7, tmin=tmin)
        assert np.all(res["tri_id"] == NO_TRI) and np.all(np.isposinf(res["t"]))
        m = c.scene.traceRaysMulti(c.o, c.d, tmax=t7, k=4, count_all=True, tmin=tmin)
        assert np.all(m["count"] == 0) and np.all(m["tri_id"] == NO_TRI)
    exp = expect(c, TMIN, bits(t7), tmax=t7)
    assert np.all(exp["count"] == 0)


@pytest.mark.parametrize("bad", [np.nan, -1.0, np.inf])
def test_invalid_tmin_is_an_invalid_ray(ctx, bad):
    c = case(ctx, "layers")
    n = c.o.shape[0]
    tmin = np.zeros(n, F)
    tmin[::3] = bad
    inv = np.zeros(n, bool)
    inv[::3] = True
    exp = expect(c, TMIN, bits(tmin))
    assert np.all(exp["count"][inv] == 0) and np.all(exp["count"][~inv] == 24) and not exp["occluded"][inv].any()
    check_all_modes(c.scene, c.o, c.d, exp, tmin=tmin)
    res = c.scene.traceRays(c.o, c.d, tmin=tmin)
    assert np.all(res["tri_id"][inv] == NO_TRI) and np.all(np.isposinf(res["t"][inv]))
    assert np.all(bits(res["u"][inv]) == 0) and np.all(bits(res["v"][inv]) == 0)
    # invalid rays are not traced: they count nothing
    for any_hit in (False, True):
        r = c.scene.traceRays(c.o[inv], c.d[inv], any_hit=any_hit, counters=True, tmin=F(bad))
        assert list(map(int, r["counters"])) == [0, 0, 0]
    r = c.scene.traceRaysMulti(c.o[inv], c.d[inv], k=4, count_all=True, counters=True, tmin=F(bad))
    assert list(map(int, r["counters"])) == [0, 0, 0] and np.all(r["count"] == 0) and np.all(r["tri_id"] == NO_TRI)


def test_any_hit_ignores_an_occluder_below_tmin(ctx):
    c = case(ctx, "layers")
    e = expect(c)
    mid = (e["t"][:, 0] + e["t"][:, 1]) * F(0.5)
    d = c.d * mid[:, None]  # segments that end between the first and the second layer
    plain = brute_filtered(c.o, d, np.inf, 0, 0, c.verts, k=2)
    assert np.all(plain["count"] >= 1) and np.all(plain["t"][:, 0] < 1) and not (plain["t"][:, 1] < 1).any()
    assert plain["occluded"].all()
    for tmin, want in ((plain["t"][:, 0], 0), (np.nextafter(plain["t"][:, 0], F(0)), 1)):
        exp = brute_filtered(c.o, d, np.inf, bits(np.ascontiguousarray(tmin)), TMIN, c.verts, k=2)
        assert np.all(exp["occluded"] == want)
        occ = c.scene.traceRays(c.o, d, any_hit=True, tmin=tmin)["occluded"]
        assert np.array_equal(occ, exp["occluded"])
    assert c.scene.traceRays(c.o, d, any_hit=True)["occluded"].all()


# ---- 4. masks ------------------------------------------------------------------------------------------
def mask_scene(ctx):
    """Three entries: Suzanne, an instance of it moved by half its extent, and Suzanne again on its own spot."""
    suz = scenes.load_mesh("suzanne")
    pos = np.concatenate([np.asarray(m["pos"], F).reshape(-1, 3) for m in suz])
    half = (pos.max(0) - pos.min(0)) * F(0.5)
    x = F([[1, 0, 0, half[0]], [0, 1, 0, half[1]], [0, 0, 1, half[2]]])
    assert len(suz) == 1
    scene = beam.IScene.create(ctx)
    (mesh,) = beam.upload_meshes(ctx, scene, suz)
    assert scene.addInstance(mesh, x) == 1
    scene.addMesh(mesh)
    scene.updateGPUScene()
    world = [suz[0], xform_mesh(x, suz[0]), suz[0]]
    return scene, mesh, suz[0], x, world


def test_entry_masks(ctx):
    scene, mesh, suz, x, world = mask_scene(ctx)
    nt = tri_vertices([suz]).shape[0]
    verts = tri_vertices(world)
    first = (0, nt, 2 * nt)
    o, d = make_batch(world, groups=6)  # 366 rays: five brute forces over 2,904 triangles
    n = o.shape[0]
    rmask = (np.arange(n) % 8).astype(np.uint32)
    assert [scene.getEntryMask(i) for i in range(3)] == [ALL_ONES] * 3
    same_as_unflagged(scene, o, d, d, ray_mask=ALL_ONES)  # default masks
    cam0 = frame(ctx, scene, 96, 96, rgb=False)
    for i, m in enumerate((1, 2, 4)):
        scene.setEntryMask(i, m)
    assert [scene.getEntryMask(i) for i in range(3)] == [1, 2, 4]
    exp = brute_filtered(o, d, np.inf, rmask, MASK, verts, first, (1, 2, 4), k=KMAX)
    assert np.all(exp["count"][rmask == 0] == 0) and exp["count"][rmask == 1].sum() > 0
    owners = np.unique(exp["tri_id"][exp["tri_id"] != NO_TRI] // nt)
    assert owners.tolist() == [0, 1, 2]  # the twin behind entry 0 shows where mask 4 is set without mask 1
    check_all_modes(scene, o, d, exp, ray_mask=rmask)
    # another assignment without a rebuild
    for i, m in enumerate((4, 1, 0x80000002)):
        scene.setEntryMask(i, m)
    exp2 = brute_filtered(o, d, np.inf, rmask, MASK, verts, first, (4, 1, 0x80000002), k=KMAX)
    assert not np.array_equal(exp2["tri_id"], exp["tri_id"])
    check_all_modes(scene, o, d, exp2, ray_mask=rmask)
    # a camera trace never reads them
    cam1 = frame(ctx, scene, 96, 96, rgb=False)
    for key in cam0:
        assert np.array_equal(cam0[key].view(np.uint32), cam1[key].view(np.uint32)), key
    assert (cam0["tri_id"] != NO_TRI).any()
    # unflagged ray queries neither
    assert_closest(scene.traceRays(o, d), brute_filtered(o, d, np.inf, 0, 0, verts, k=1))
    # the masks survive a refit that moves the instance
    x2 = x.copy()
    x2[:, 3] *= F(0.5)
    scene.setInstanceTransform(1, x2)
    scene.refitGPUScene()
    world2 = [suz, xform_mesh(x2, suz), suz]
    exp3 = brute_filtered(o, d, np.inf, rmask, MASK, tri_vertices(world2), first, (4, 1, 0x80000002), k=KMAX)
    check_all_modes(scene, o, d, exp3, ray_mask=rmask)
    # removing entry 0: the masks move down with their entries; a new entry has all ones
    scene.removeInstance(0)
    scene.addMesh(mesh)
    assert [scene.getEntryMask(i) for i in range(3)] == [1, 0x80000002, ALL_ONES]
    scene.updateGPUScene()
    assert [scene.getEntryMask(i) for i in range(3)] == [1, 0x80000002, ALL_ONES]
    world4 = [xform_mesh(x2, suz), suz, suz]
    exp4 = brute_filtered(o, d, np.inf, rmask, MASK, tri_vertices(world4), first, (1, 0x80000002, ALL_ONES), k=KMAX)
    check_all_modes(scene, o, d, exp4, ray_mask=rmask)
    scene.destroy()


# ---- 5. edges ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 15, 16, 17])
def test_batch_edges_write_nothing_past_n(ctx, n):
    import torch
    c = case(ctx, "suzanne")
    dev = torch.device("cuda", ctx.device)
    first = expect(c)
    idx = np.flatnonzero(first["count"] > 1)[:n]
    assert idx.size == n
    ids = first["tri_id"][idx, 0]
    flags = SKIP | FRONT
    exp = brute_filtered(c.o[idx], c.d[idx], np.inf, ids, flags, c.verts, k=KMAX)
    rays = np.zeros((n, 8), F)
    rays[:, 0:3], rays[:, 3], rays[:, 4:7] = c.o[idx], np.inf, c.d[idx]
    rays.view(np.uint32)[:, 7] = ids
    r_dev = torch.from_numpy(rays).to(dev)
    hits = torch.full((n * 4 + 64, 4), -7.5, dtype=torch.float32, device=dev)
    one = torch.full((n + 64, 4), -7.5, dtype=torch.float32, device=dev)
    occ = torch.full((n + 64,), 9, dtype=torch.uint8, device=dev)
    counts = torch.full((n + 64,), -3, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    assert c.scene.traceRaysDevice(r_dev.data_ptr(), n, one.data_ptr(), flags=flags) == 0
    assert c.scene.traceRaysDevice(r_dev.data_ptr(), n, occ.data_ptr(), any_hit=True, flags=flags) == 0
    assert c.scene.traceRaysMultiDevice(r_dev.data_ptr(), n, 4, hits.data_ptr(), counts.data_ptr(), flags | ALL) == 0
    ctx.sync()
    h, h1, oc, cn = hits.cpu().numpy(), one.cpu().numpy(), occ.cpu().numpy(), counts.cpu().numpy()
    assert np.all(h[n * 4:] == F(-7.5)) and np.all(h1[n:] == F(-7.5)) and np.all(oc[n:] == 9) and np.all(cn[n:] == -3)
    h = h[:n * 4].reshape(n, 4, 4)
    got = {"t": h[..., 0], "u": h[..., 1], "v": h[..., 2], "tri_id": h.view(np.uint32)[..., 3], "count": cn[:n].view(np.uint32)}
    assert_multi(got, exp, 4, True)
    assert_closest({"t": h1[:n, 0], "u": h1[:n, 1], "v": h1[:n, 2], "tri_id": h1.view(np.uint32)[:n, 3]}, exp)
    assert np.array_equal(oc[:n], exp["occluded"])


def test_small_grid_strides_over_the_batches(ctx):
    c = case(ctx, "suzanne")
    small = beam.Context(device=0, params={"trace_grid": 1})  # 4 waves: about 15 batches each
    scene, keep = build(small, c.meshes)
    check_all_modes(scene, c.o, c.d, expect(c, BACK), cull="back")
    tmin = F(0.5)
    check_all_modes(scene, c.o, c.d, expect(c, TMIN | FRONT, int(tmin.view(np.uint32))), tmin=tmin, cull="front")
    scene.destroy()
    small.close()


def test_empty_built_scene(ctx):
    c = case(ctx, "suzanne")
    scene, keep = build(ctx, [])
    for kw in ({"cull": "back"}, {"skip_tri": 3}, {"tmin": 0.5}, {"ray_mask": ALL_ONES}, {"cull": "front", "ray_mask": 1}):
        res = scene.traceRays(c.o[:100], c.d[:100], counters=True, **kw)
        assert np.all(res["tri_id"] == NO_TRI) and np.all(np.isposinf(res["t"])) and int(res["counters"][2]) == 0
        assert not scene.traceRays(c.o[:100], c.d[:100], any_hit=True, **kw)["occluded"].any()
        m = scene.traceRaysMulti(c.o[:100], c.d[:100], k=4, count_all=True, **kw)
        assert np.all(m["tri_id"] == NO_TRI) and np.all(m["count"] == 0)
    scene.destroy()


@pytest.mark.parametrize("ntri", [1, 2, 3, 4, 5])
def test_tiny_scenes(ctx, ntri):
    meshes, eyes, o, d = tiny_scene(ntri)
    verts = tri_vertices(meshes)
    scene, keep = build(ctx, meshes)
    n = o.shape[0]
    for flags, pad, kw in ((BACK, 0, {"cull": "back"}), (FRONT | SKIP, np.arange(n) % ntri, None),
                           (TMIN, bits(np.full(n, 1.0, F)), {"tmin": 1.0})):
        exp = brute_filtered(o, d, np.inf, pad, flags, verts, k=KMAX)
        kw = {"cull": "front", "skip_tri": np.arange(n) % ntri} if kw is None else kw
        check_all_modes(scene, o, d, exp, **kw)
    scene.setEntryMask(0, 2)
    rmask = (np.arange(n) % 4).astype(np.uint32)
    exp = brute_filtered(o, d, np.inf, rmask, MASK, verts, (0,), (2,), k=KMAX)
    check_all_modes(scene, o, d, exp, ray_mask=rmask)
    scene.destroy()


def test_deep_scene_filters_run_through_the_overflow_area():
    _, dup, leaf = ds.scene_of("deep+dup-leaf1")
    dctx = beam.Context(device=0, leaf_size=leaf)
    meshes = ds.deep_meshes(dup)
    scene, keep = build(dctx, meshes)
    o, d = ds.ray_batch()
    verts = tri_vertices(meshes)
    assert o.shape[0] * verts.shape[0] < 5e7
    plain = brute_filtered(o, d, np.inf, 0, 0, verts, k=KMAX)
    ids = plain["tri_id"][:, 0]  # skipping the closest hit: the traversal goes on past it, among 1,024 twins
    exp = brute_filtered(o, d, np.inf, ids, SKIP | BACK, verts, k=KMAX)
    assert (exp["count"] > 0).any() and not np.array_equal(exp["tri_id"], plain["tri_id"])
    check_all_modes(scene, o, d, exp, skip_tri=ids, cull="back")
    same_as_unflagged(scene, o, d, d, skip_tri=NO_TRI)
    scene.destroy()
    dctx.close()


def test_query_after_refit(ctx):
    c = case(ctx, "suzanne")
    scene = beam.IScene.create(ctx)
    meshes = beam.upload_meshes(ctx, scene, c.meshes)
    scene.updateGPUScene()
    scene.setEntryMask(0, 6)
    moved = []
    for m in c.meshes:
        p = np.asarray(m["pos"], F)
        q = p.copy()
        q[:, 1] += F(0.03) * np.sin(F(8.0) * p[:, 0] + F(1.0)).astype(F)
        moved.append(dict(m, pos=q))
    for m, mv in zip(meshes, moved):
        assert m.setVertexData(mv["pos"], mv["pos"].shape[0], 3, beam.VERTEX_DATA_POSITION) == 0
    scene.refitGPUScene()
    verts = tri_vertices(moved)
    exp = brute_filtered(c.o, c.d, np.inf, 0, FRONT, verts, k=KMAX)
    assert not np.array_equal(exp["tri_id"], expect(c, FRONT)["tri_id"])
    check_all_modes(scene, c.o, c.d, exp, cull="front")
    rmask = (np.arange(c.o.shape[0]) % 8).astype(np.uint32)
    expm = brute_filtered(c.o, c.d, np.inf, rmask, MASK | BACK, verts, (0,), (6,), k=KMAX)
    check_all_modes(scene, c.o, c.d, expm, ray_mask=rmask, cull="back")
    scene.destroy()


# ---- 6. errors -----------------------------------------------------------------------------------------
def test_errors(ctx):
    import torch
    c = case(ctx, "suzanne")
    dev = torch.device("cuda", ctx.device)
    n = 64
    rays = torch.zeros((n, 8), dtype=torch.float32, device=dev)
    out = torch.zeros((n * 16, 4), dtype=torch.float32, device=dev)
    cnt = torch.zeros((n,), dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    rp, op, cp = rays.data_ptr(), out.data_ptr(), cnt.data_ptr()
    s = c.scene
    pads = (SKIP, TMIN, MASK)
    for f in (BACK, FRONT) + pads:
        for g in (0, BACK, FRONT):
            if f in (BACK, FRONT) and g and g != f:
                continue
            assert s.traceRaysDevice(rp, n, op, flags=f | g) == 0
            assert s.traceRaysDevice(rp, n, op, any_hit=True, flags=f | g) == 0
            assert s.traceRaysMultiDevice(rp, n, 4, op, cp, f | g) == 0
            assert s.traceRaysMultiDevice(rp, n, 4, op, cp, f | g | ALL) == 0
    bad = [BACK | FRONT, SKIP | TMIN, SKIP | MASK, TMIN | MASK, SKIP | TMIN | MASK, BACK | FRONT | SKIP, 0x200, 0x8, 0x4]
    for f in bad:
        assert s.traceRaysDevice(rp, n, op, flags=f) == BAD, hex(f)
        assert s.traceRaysDevice(rp, n, op, any_hit=True, flags=f) == BAD, hex(f)
        assert s.traceRaysMultiDevice(rp, n, 4, op, cp, f) == BAD, hex(f)
        assert s.traceRaysMultiDevice(rp, n, 4, op, cp, f | ALL) == BAD, hex(f)
    for f in (1, 2, 0x80000000):
        assert s.traceRaysDevice(rp, n, op, flags=f) == BAD and s.traceRaysDevice(rp, n, op, flags=f | BACK) == BAD
    for f in (2, 3, 0x80000000):
        assert s.traceRaysMultiDevice(rp, n, 4, op, cp, f | TMIN) == BAD
    counters = np.zeros(3, np.uint64)
    assert s.traceRaysDevice(rp, n, op, counters=counters, flags=BACK | FRONT) == BAD
    assert s.traceRaysMultiDevice(rp, n, 4, op, cp, SKIP | MASK, counters) == BAD
    # point queries have no filter flags
    pts = torch.zeros((n, 4), dtype=torch.float32, device=dev)
    assert ctx.lib.bm_scene_closest_points(s.h, pts.data_ptr(), n, BACK, op) == BAD
    ctx.sync()
    unbuilt = beam.IScene.create(ctx)
    assert unbuilt.traceRaysDevice(rp, n, op, flags=MASK) == _lib.ERROR_NOT_BUILT
    unbuilt.destroy()
    # entry masks: index errors
    lib = ctx.lib
    m = C.c_uint32(7)
    assert lib.bm_scene_set_entry_mask(s.h, 0, 5) == 0 and lib.bm_scene_get_entry_mask(s.h, 0, m) == 0 and m.value == 5
    assert lib.bm_scene_set_entry_mask(s.h, 0, ALL_ONES) == 0
    assert lib.bm_scene_set_entry_mask(s.h, 1, 5) == BAD and lib.bm_scene_get_entry_mask(s.h, 1, m) == BAD
    assert lib.bm_scene_set_entry_mask(s.h, ALL_ONES, 5) == BAD
    assert lib.bm_scene_get_entry_mask(s.h, 0, None) == BAD
    assert lib.bm_scene_set_entry_mask(None, 0, 5) == BAD and lib.bm_scene_get_entry_mask(None, 0, m) == BAD
    with pytest.raises(beam.BeamError):
        s.setEntryMask(1, 1)
    with pytest.raises(beam.BeamError):
        s.traceRays(c.o, c.d, skip_tri=1, tmin=0.5)
    tiny = [{"pos": F([[0, 0, 1], [1, 0, 1], [0, 1, 1]]), "nrm": F([[0, 0, 1]] * 3), "idx": np.uint32([0, 1, 2])}]
    for kw in ({"reference_kd": True}, {"reference_hash": True}, {"bvh_width": 2}):
        other = beam.Context(device=0, **kw)
        sc, keep = build(other, tiny)
        for f in (BACK, SKIP, TMIN, MASK):
            assert sc.traceRaysDevice(rp, n, op, flags=f) == BAD, kw
            assert sc.traceRaysMultiDevice(rp, n, 4, op, cp, f | ALL) == BAD, kw
        sc.setEntryMask(0, 3)  # scene state: no query needed
        assert sc.getEntryMask(0) == 3
        sc.destroy()
        other.close()


# ---- 7. torch ------------------------------------------------------------------------------------------
def test_torch_chain_stays_on_the_device():
    """trace -> hitAttributes(position) -> next rays from the hit points with pad = tri_id -> trace, on one stream
    with nothing waiting, equal to the same chain through numpy and to the brute force."""
    import torch
    from test_gpu_attrs import expected
    meshes = scenes.load_mesh("suzanne")
    verts = tri_vertices(meshes)
    o, d = make_batch(meshes)
    dev = torch.device("cuda", 0)
    tctx = beam.Context(device=0, stream=torch.cuda.current_stream(dev).cuda_stream)
    scene, keep = build(tctx, meshes)
    n = o.shape[0]
    packed = np.zeros((n, 8), F)
    packed[:, 0:3], packed[:, 3], packed[:, 4:7] = o, np.inf, d
    d2 = F(np.random.default_rng(43).normal(size=(n, 3)))
    rays = torch.from_numpy(packed).to(dev)
    d2_dev = torch.from_numpy(d2).to(dev)
    # no synchronisation from here to the end of the chain
    first = scene.traceRays(rays)
    (pos,) = scene.hitAttributes(first["hits"], [(beam.VERTEX_DATA_POSITION, 3)])
    second = scene.traceRays(pos, d2_dev, skip_tri=first["tri_id"])
    multi = scene.traceRaysMulti(pos, d2_dev, k=4, skip_tri=first["tri_id"], cull="back")
    packed2 = torch.zeros((n, 8), dtype=torch.float32, device=dev)
    packed2[:, 0:3], packed2[:, 3], packed2[:, 4:7] = pos, float("inf"), d2_dev
    packed2.view(torch.int32)[:, 7] = first["tri_id"]
    third = scene.traceRays(packed2, flags=SKIP)
    assert second["hits"].is_cuda and multi["hits"].is_cuda
    torch.cuda.synchronize()
    h1 = first["hits"].cpu().numpy()
    ids = h1.view(np.uint32)[:, 3].copy()
    hit = ids != NO_TRI
    assert 200 < hit.sum() < n
    p = pos.cpu().numpy()
    assert np.array_equal(p.view(np.uint32), expected(meshes, h1, beam.VERTEX_DATA_POSITION, 3).view(np.uint32))
    # the numpy route from the same hit points
    host = scene.traceRays(p, d2, skip_tri=ids)
    got = {key: second[key].cpu().numpy() for key in ("t", "u", "v")}
    got["tri_id"] = second["tri_id"].cpu().numpy().view(np.uint32)
    for key in got:
        assert np.array_equal(got[key].view(np.uint32), host[key].view(np.uint32)), key
    assert torch.equal(third["hits"].view(torch.int32), second["hits"].view(torch.int32))
    exp = brute_filtered(p, d2, np.inf, ids, SKIP, verts, k=4)
    assert_closest(got, exp)
    assert not (got["tri_id"][hit] == ids[hit]).any()
    hm = multi["hits"].cpu().numpy()
    gm = {"t": hm[..., 0], "u": hm[..., 1], "v": hm[..., 2], "tri_id": hm.view(np.uint32)[..., 3],
          "count": multi["count"].cpu().numpy().view(np.uint32)}
    assert_multi(gm, brute_filtered(p, d2, np.inf, ids, SKIP | BACK, verts, k=4), 4)
    scene.destroy()
    tctx.close()
