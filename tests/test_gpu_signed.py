"""GPU checks of signed-distance and occupancy queries (bm_scene_signed_distances).

The yardstick is tests/test_signed_abi.py: brute_force_signed, the crossing parity of the ray (p, D_j, +inf) over
ALL triangles by the numpy restatement of the ray/triangle function, and the closest-point brute force with the
sign on t. The traversal prunes and skips boxes, the brute force does not; t, u, v (as bit images), tri_id, the
occupancy byte and the votes must be equal. On the same context the record must also equal closestPoints' and the
votes traceRaysMulti(k=0, count_all=True) & 1. No expected value comes from the library.
"""
from types import SimpleNamespace

import numpy as np
import pytest

import deep_scenes
from raytracercuda_amd import _lib, beam, scenes
from test_gpu_attrs import assert_rows, expected
from test_gpu_points import bits, build, make_points, soup, take, tri_vertices
from test_instances_abi import MIRROR, rotation, xform_mesh
from test_multihit_abi import tri_hit
from test_signed_abi import (DIRS, NO_TRI, both_votes, brute_force_signed, cube_inside, cube_verts, grid_points, icosphere_verts,
                             octahedron_verts, shell_points)

pytestmark = pytest.mark.gpu

F = np.float32
MISS = np.uint32(NO_TRI)
QUAD_LDS = 24  # stack entries a query keeps in LDS (bm_trace_quad.h); beyond: the global overflow area
POS, FACE = beam.VERTEX_DATA_POSITION, beam.ATTR_MESH_FACE
SHIFT = F([1000, -2000, 500])
SIGN = np.uint32(0x80000000)
FLT_MAX = np.finfo(np.float32).max


def assert_signed(res, exp, dist, what):
    """The query's result against the brute force's: the votes, the byte or the record's bit images."""
    bad = res["votes"] != exp["votes"]
    assert not bad.any(), f"{what}: votes differ on {int(bad.sum())} points, first {np.flatnonzero(bad)[:5]}"
    if not dist:
        assert np.array_equal(res["inside"], exp["inside"].astype(bool)), what
        return
    bad = res["tri_id"] != exp["tri_id"]
    assert not bad.any(), f"{what}: tri_id differs on {int(bad.sum())} points, first {np.flatnonzero(bad)[:5]}"
    for k in ("t", "u", "v"):
        diff = bits(res[k]) != bits(exp[k])
        assert not diff.any(), f"{what}: {k} differs on {int(diff.sum())} points, first {np.flatnonzero(diff)[:5]}"


def check(scene, p, rmax, verts, what, exps=None, cross=True):
    """Both modes, one vote and three, over points p (n,3) with rmax against the brute force and, with `cross`,
    against closestPoints and traceRaysMulti on the same scene. Returns {vote3: brute force's answers}."""
    n = p.shape[0]
    rmax = np.ascontiguousarray(np.broadcast_to(np.asarray(rmax, F), (n,)))
    exps = exps or both_votes(p, rmax, verts)
    for v3 in (False, True):
        exp = exps[v3]
        res = scene.signedDistance(p, rmax, vote3=v3, votes=True)
        assert_signed(res, exp, True, f"{what}, distance, vote3={v3}")
        plain = scene.signedDistance(p, rmax, vote3=v3)  # votes_dev NULL
        assert "votes" not in plain and np.array_equal(bits(plain["t"]), bits(res["t"]))
        assert np.array_equal(plain["tri_id"], res["tri_id"])
        occ = scene.occupancy(p, vote3=v3, votes=True)
        valid = np.isfinite(p).all(axis=1)
        oexp = exp if valid.all() and (rmax > 0).all() else brute_force_signed(p, rmax, verts, distance=False, vote3=v3)
        assert_signed(occ, oexp, False, f"{what}, occupancy, vote3={v3}")
        assert np.array_equal(scene.occupancy(p, vote3=v3)["inside"], occ["inside"])
    if cross:
        ref = scene.closestPoints(p, rmax)
        got = scene.signedDistance(p, rmax, vote3=True, votes=True)
        assert np.array_equal(bits(got["t"]) & ~SIGN, bits(ref["t"])), what
        assert np.array_equal(bits(got["u"]), bits(ref["u"])) and np.array_equal(bits(got["v"]), bits(ref["v"]))
        assert np.array_equal(got["tri_id"], ref["tri_id"])
        with np.errstate(all="ignore"):
            valid = np.isfinite(p).all(axis=1) & (rmax > 0)
        votes = np.zeros(n, np.uint32)
        for j in range(3):
            cnt = scene.traceRaysMulti(p, np.broadcast_to(DIRS[j], (n, 3)), np.inf, k=0, count_all=True)["count"]
            votes += np.where(valid, cnt & 1, 0).astype(np.uint32)
            assert np.array_equal(np.where(valid, cnt, 0), exps[True]["counts"][:, j]), (what, j)
        assert np.array_equal(got["votes"], votes.astype(np.uint8)), what
        assert np.array_equal(np.signbit(got["t"]), votes >= 2)
    return exps


_CASES = {}


def case(ctx, name, n=1000):
    """Mesh, GPU scene, the point set and the brute force's answers for it — computed once per module run."""
    if name not in _CASES:
        meshes = scenes.load_mesh(name)
        scene, keep = build(ctx, meshes)
        pts = make_points(meshes, n, 29)
        verts = tri_vertices(meshes)
        exps = both_votes(pts, np.inf, verts)
        _CASES[name] = SimpleNamespace(meshes=meshes, scene=scene, keep=keep, pts=pts, verts=verts, exps=exps)
    return _CASES[name]


def teardown_module(module):
    for k in _CASES.values():
        k.scene.destroy()
    _CASES.clear()


# ---- 1. small scenes -------------------------------------------------------------------------------------
@pytest.mark.parametrize("ntri", [0, 1, 4, 5, 17])
def test_small_scenes(ctx, ntri):
    rng = np.random.default_rng(500 + ntri)
    base = rng.uniform(-1, 1, (ntri, 1, 3))
    verts = F(base + rng.uniform(-0.8, 0.8, (ntri, 3, 3)))
    scene, keep = build(ctx, soup(verts) if ntri else [])
    p = F(rng.uniform(-2, 2, (203, 3)))
    if ntri == 0:  # a built scene with no triangles: every point outside
        for v3 in (False, True):
            res = scene.signedDistance(p, vote3=v3, votes=True, counters=True)
            assert np.isposinf(res["t"]).all() and (res["tri_id"] == MISS).all() and not res["votes"].any()
            assert (bits(res["u"]) == 0).all() and (bits(res["v"]) == 0).all()
            assert [int(x) for x in res["counters"]] == [0, 0, 0, 0]
            occ = scene.occupancy(p, vote3=v3, votes=True)
            assert not occ["inside"].any() and not occ["votes"].any()
    else:
        exps = check(scene, p, np.inf, verts, f"{ntri} triangles")
        assert exps[True]["votes"].max() >= 1  # open soups: some rays cross once
    scene.destroy()


# ---- 2. closed meshes on the grid --------------------------------------------------------------------------
def test_cube_grid_surface_points_included(ctx):
    verts = cube_verts()
    p = grid_points()
    scene, keep = build(ctx, soup(verts))
    exps = check(scene, p, np.inf, verts, "cube grid")
    inside, on = cube_inside(p)
    assert on.sum() == 1538 and np.array_equal(exps[False]["inside"][~on].astype(bool), inside[~on])
    assert (exps[True]["t"][on] == 0).all()  # +0 or -0: compared above as bits
    # sdfGrid: the same cell centres through the per-point call, reshaped
    import torch
    lo, hi, dims = (-1.5, -1.25, -1.0), (1.5, 1.75, 2.0), (7, 5, 6)
    cell = (F(hi) - F(lo)) / F(dims)
    idx = np.stack(np.meshgrid(*(np.arange(d, dtype=F) for d in dims), indexing="ij"), axis=-1)
    centres = (F(lo) + (idx + F(0.5)) * cell).reshape(-1, 3)
    grid = scene.sdfGrid(lo, hi, dims)
    ctx.sync()
    assert isinstance(grid, torch.Tensor) and tuple(grid.shape) == dims and grid.dtype == torch.float32
    per_point = scene.signedDistance(centres, vote3=True)["t"].reshape(dims)
    assert np.array_equal(bits(grid.cpu().numpy()), bits(per_point))
    assert np.array_equal(bits(per_point), bits(brute_force_signed(centres, np.inf, verts, vote3=True)["t"].reshape(dims)))
    band = scene.sdfGrid(lo, hi, dims, rmax=0.2, vote3=False)
    ctx.sync()
    b = band.cpu().numpy()
    assert np.isinf(b).any() and np.array_equal(np.signbit(b), np.signbit(per_point))
    scene.destroy()


def test_octahedron_and_icosphere(ctx):
    verts = octahedron_verts()
    scene, keep = build(ctx, soup(verts))
    check(scene, grid_points()[::3], np.inf, verts, "octahedron grid")
    scene.destroy()
    verts = icosphere_verts(2)
    p, inside = shell_points(2000)
    scene, keep = build(ctx, soup(verts))
    exps = check(scene, p, np.inf, verts, "icosphere")
    assert np.array_equal(exps[False]["inside"].astype(bool), inside)
    assert np.array_equal(exps[True]["inside"].astype(bool), inside)
    scene.destroy()


# ---- 3. open meshes ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["bunny", "suzanne"])
def test_open_meshes_mixed_votes_match(ctx, name):
    k = case(ctx, name)
    assert k.pts.shape[0] == 1000
    v = k.exps[True]["votes"]
    assert ((v == 1) | (v == 2)).sum() >= 1, "an open mesh: some point has mixed votes"
    assert (v == 3).sum() > 50 and (v == 0).sum() > 300
    check(k.scene, k.pts, np.inf, k.verts, name, k.exps)


def test_translated_suzanne(ctx):
    base = scenes.load_mesh("suzanne")
    moved = [dict(m, pos=np.asarray(m["pos"], F).reshape(-1, 3) + SHIFT) for m in base]
    verts = tri_vertices(moved)
    p = make_points(moved, 1000, 31)
    scene, keep = build(ctx, moved)
    exps = check(scene, p, np.inf, verts, "translated suzanne")
    assert (exps[True]["votes"] == 3).sum() > 50
    scene.destroy()


def test_mesh_added_twice_flips_back(ctx):
    verts = icosphere_verts(2)
    p, inside = shell_points(600, seed=12)
    scene, keep = build(ctx, soup(verts) + soup(verts))
    both = np.concatenate([verts, verts])
    exps = check(scene, p, np.inf, both, "icosphere twice")
    assert not exps[False]["inside"].any() and not exps[True]["inside"].any()
    assert (exps[True]["counts"][inside] == 2).all()
    scene.destroy()


# ---- 4. instances and refit, chained into hit attributes ----------------------------------------------------------
def chain(scene, meshes, p, verts, what):
    exps = check(scene, p, np.inf, verts, what)
    res = scene.signedDistance(p, vote3=True)
    ref = scene.closestPoints(p)
    hits, plain = np.zeros((p.shape[0], 4), F), np.zeros((p.shape[0], 4), F)
    for h, r in ((hits, res), (plain, ref)):
        h[:, 0], h[:, 1], h[:, 2] = r["t"], r["u"], r["v"]
        h.view(np.uint32)[:, 3] = r["tri_id"]
    assert np.signbit(hits[:, 0]).sum() > 20
    pos, face = scene.hitAttributes(hits, [(POS, 3), (FACE, 2)])
    pos0, face0 = scene.hitAttributes(plain, [(POS, 3), (FACE, 2)])
    assert_rows(pos, pos0, what + ": closest point")  # the sign on t changes nothing downstream
    assert_rows(face, face0, what + ": owner")
    assert_rows(pos, expected(meshes, hits, POS, 3), what + ": closest point, yardstick")
    return exps, face


def test_instances_chained_into_hit_attributes(ctx):
    verts0 = icosphere_verts(2)
    base = soup(verts0)[0]
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
    q, _ = shell_points(300, seed=13)
    centres = np.float64([[0, 0, 0], [3.5, -0.25, 2.0], [-3.25, 0.5, -1.0]])
    p = F(np.concatenate([q.astype(np.float64) + c for c in centres]))
    exps, face = chain(scene, pre, p, verts, "instances")
    ins = exps[True]["inside"].astype(bool)
    assert set(face[ins, 0].tolist()) == {0, 1, 2}  # points inside each of the three copies
    scene.destroy()


def test_after_refit_chained_into_hit_attributes(ctx):
    verts0 = icosphere_verts(2)
    base = soup(verts0)
    scene = beam.IScene.create(ctx)
    meshes = beam.upload_meshes(ctx, scene, base)
    scene.updateGPUScene()
    p0 = np.asarray(base[0]["pos"], F).reshape(-1, 3)
    q = p0.copy()  # scaled and sheared
    q[:, 0] = p0[:, 0] * F(1.25) + p0[:, 1] * F(0.5)
    q[:, 1] = p0[:, 1] * F(0.75)
    q[:, 2] = p0[:, 2] * F(1.5) + p0[:, 0] * F(0.25)
    moved = [dict(base[0], pos=q)]
    assert meshes[0].setVertexData(q, q.shape[0], 3, POS) == 0
    scene.refitGPUScene()
    verts = tri_vertices(moved)
    p = make_points(moved, 600, 37)
    exps, _ = chain(scene, moved, p, verts, "after refit")
    assert 50 < exps[True]["inside"].sum() < 550
    scene.destroy()


# ---- 5. rmax bands -----------------------------------------------------------------------------------------------
def test_rmax_bands_keep_their_sign(ctx):
    verts = icosphere_verts(2)
    p, inside = shell_points(1200, seed=14)
    rng = np.random.default_rng(15)
    rmax = F(rng.choice([0.02, 0.1, 0.3, np.inf], 1200))
    scene, keep = build(ctx, soup(verts))
    exps = check(scene, p, rmax, verts, "bands")
    t = exps[True]["t"]
    assert np.isneginf(t).sum() > 100 and np.isposinf(t).sum() > 100  # beyond rmax on both sides of the surface
    assert (np.isfinite(t) & inside).sum() > 100 and (np.isfinite(t) & ~inside).sum() > 100
    assert np.array_equal(np.signbit(t), inside)
    assert (exps[True]["tri_id"][np.isinf(t)] == MISS).all()
    scene.destroy()


# ---- 6. invalid points -------------------------------------------------------------------------------------------
def test_invalid_points_among_valid_ones_and_alone(ctx):
    k = case(ctx, "suzanne")
    n = 400
    p, rmax = k.pts[:n].copy(), np.full(n, np.inf, F)
    kind = np.arange(n) % 8  # 0, 1: valid
    p[kind == 2, 0] = np.nan
    p[kind == 3, 1] = np.inf
    p[kind == 4, 2] = -np.inf
    rmax[kind == 5] = np.nan
    rmax[kind == 6] = 0.0
    rmax[kind == 7] = -1.0
    invalid = kind >= 2
    exps = check(k.scene, p, rmax, k.verts, "with invalid points")
    for v3 in (False, True):
        e = exps[v3]
        assert np.isposinf(e["t"][invalid]).all() and not e["votes"][invalid].any()
        res = k.scene.signedDistance(p[invalid], rmax[invalid], vote3=v3, votes=True, counters=True)
        assert [int(x) for x in res["counters"]] == [0, 0, 0, 0]  # invalid points count nothing
        assert np.isposinf(res["t"]).all() and (res["tri_id"] == MISS).all() and not res["votes"].any()
        assert (bits(res["u"]) == 0).all() and (bits(res["v"]) == 0).all()
    bad_p = kind[invalid] <= 4
    occ = k.scene.occupancy(p[invalid], vote3=True, votes=True)
    assert not occ["inside"][bad_p].any() and not occ["votes"][bad_p].any()
    assert occ["votes"][~bad_p].any()  # occupancy does not read rmax


# ---- 7. batch edges --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 15, 16, 17, 63, 64, 65])
def test_batch_edges_write_nothing_past_n(ctx, n):
    import torch
    k = case(ctx, "suzanne")
    dev = torch.device("cuda", ctx.device)
    packed = np.zeros((n, 4), F)
    packed[:, 0:3], packed[:, 3] = k.pts[:n], np.inf
    p_dev = torch.from_numpy(packed).to(dev)
    hits = torch.full((n + 64, 4), -7.5, dtype=torch.float32, device=dev)
    flags = torch.full((n + 256,), 77, dtype=torch.uint8, device=dev)
    votes = torch.full((n + 256 + 1,), 55, dtype=torch.uint8, device=dev)[1:]  # votes_dev needs no alignment
    ovotes = torch.full((n + 256 + 3,), 66, dtype=torch.uint8, device=dev)[3:]
    torch.cuda.synchronize()
    assert votes.data_ptr() % 2 == 1
    v3 = _lib.SIGNED_VOTE3
    assert k.scene.signedDistancesDevice(p_dev.data_ptr(), n, hits.data_ptr(), flags=v3, votes=votes.data_ptr()) == 0
    assert k.scene.signedDistancesDevice(p_dev, n, flags, mode=_lib.SIGNED_OCCUPANCY, flags=v3, votes=ovotes) == 0
    ctx.sync()
    h, a, v, ov = hits.cpu().numpy(), flags.cpu().numpy(), votes.cpu().numpy(), ovotes.cpu().numpy()
    assert np.all(h[n:] == F(-7.5)) and np.all(a[n:] == 77) and np.all(v[n:] == 55) and np.all(ov[n:] == 66)
    exp = take(k.exps[True], np.arange(n))
    got = {"t": h[:n, 0], "u": h[:n, 1], "v": h[:n, 2], "tri_id": h.view(np.uint32)[:n, 3], "votes": v[:n]}
    assert_signed(got, exp, True, f"n = {n}")
    assert np.array_equal(a[:n], exp["inside"]) and np.array_equal(ov[:n], exp["votes"])


@pytest.mark.parametrize("grid", [1, 2])
def test_small_grid_strides_over_the_batches(ctx, grid):
    k = case(ctx, "suzanne")
    small = beam.Context(device=0, params={"trace_grid": grid})
    scene, keep = build(small, k.meshes)
    check(scene, k.pts, np.inf, k.verts, f"trace_grid {grid}", k.exps, cross=False)
    scene.destroy()
    small.close()


# ---- 8. the stack's overflow area --------------------------------------------------------------------------------
def parity_walk(rec, verts, gid, p, d):
    """The parity traversal restated over exported BVH4 records (bm_signed.hip parity_visit, quad_parity): the
    ray query's box test at bound +inf in float32, the kept children in slot order. Returns (crossings, node
    records fetched, triangle tests, the most stack entries held at once)."""
    with np.errstate(all="ignore"):
        inv = F(1) / d
    stack, cur, nodes, tests, crossings, deepest = [], 0, 0, 0, 0, 0
    while True:
        if cur is not None and cur & 0x80000000:
            first, cnt = cur & 0x07FFFFFF, ((cur >> 27) & 15) + 1
            g = gid[first:first + cnt]
            t, _, _, ok = tri_hit(p[None, :], d[None, :], verts[g, 0], verts[g, 1], verts[g, 2])
            with np.errstate(all="ignore"):
                crossings += int((ok & (t > F(0)) & (t < FLT_MAX)).sum())
            tests += cnt
            cur = None
        if cur is None:
            if not stack:
                return crossings, nodes, tests, deepest
            cur = stack.pop()
            continue
        nodes += 1
        box = rec[cur, :24].view(F).reshape(6, 4)
        ref = rec[cur, 24:28]
        with np.errstate(all="ignore"):
            tl = (box[0:3] - p[:, None]) * inv[:, None]
            th = (box[3:6] - p[:, None]) * inv[:, None]
            tn = np.fmax(np.fmax(np.fmin(tl[0], th[0]), np.fmin(tl[1], th[1])), np.fmin(tl[2], th[2]))
            tf = np.fmin(np.fmin(np.fmax(tl[0], th[0]), np.fmax(tl[1], th[1])), np.fmax(tl[2], th[2]))
            kept = [int(ref[c]) for c in range(4) if tn[c] <= tf[c] and tf[c] >= 0]
        assert 0xFFFFFFFF not in kept  # an empty slot's NaN box is never entered
        cur = kept[0] if kept else None
        stack.extend(reversed(kept[1:]))
        deepest = max(deepest, len(stack))


def test_deep_chain_uses_the_overflow_area(ctx):
    meshes = deep_scenes.deep_meshes()
    verts = tri_vertices(meshes)
    rng = np.random.default_rng(41)
    # points before the chain along each direction, so that the rays run through every sibling's box, and around
    back = np.concatenate([F([300, 300, 300]) - F(rng.uniform(2500, 4500, (12, 1))) * DIRS[j] for j in range(3)])
    p = F(np.concatenate([back + F(rng.uniform(-200, 200, back.shape)), rng.uniform(-3000, 3000, (29, 3))]))
    n = p.shape[0]
    scene, keep = build(ctx, meshes)
    rec, tris, _, _ = scene.export()
    gid = tris[:, 3].astype(np.int64)
    deepest, nodes, tests = 0, 0, 0
    walked = np.zeros((n, 3), np.uint32)
    for i in range(n):
        for j in range(3):
            c, nn, tt, dp = parity_walk(rec, verts, gid, p[i], DIRS[j])
            walked[i, j], nodes, tests, deepest = c, nodes + nn, tests + tt, max(deepest, dp)
    print(f"deep chain: {verts.shape[0]} triangles, deepest parity stack {deepest} entries (LDS holds {QUAD_LDS}), "
          f"{nodes / (3 * n):.1f} node records and {tests / (3 * n):.1f} triangle tests per ray")
    assert deepest >= QUAD_LDS + 1, f"the overflow path does not run: deepest stack {deepest}"
    exps = check(scene, p, np.inf, verts, "deep chain")
    assert np.array_equal(walked, exps[True]["counts"])  # the walk skips no crossing
    assert (exps[True]["votes"] > 0).sum() >= 5
    res = scene.signedDistance(p, vote3=True, votes=True, counters=True)
    assert_signed(res, exps[True], True, "deep chain, counting kernel")
    assert (int(res["counters"][2]), int(res["counters"][3])) == (nodes, tests)  # the walk's records and tests
    occ = scene.occupancy(p, vote3=True, votes=True)
    assert_signed(occ, exps[True], False, "deep chain, occupancy")
    scene.destroy()


# ---- 9. counters -------------------------------------------------------------------------------------------------
def test_counters(ctx):
    import torch
    k = case(ctx, "suzanne")
    n = k.pts.shape[0]
    ref = k.scene.closestPoints(k.pts, counters=True)["counters"]
    multi = np.zeros(2, np.int64)
    for j in range(3):
        c = k.scene.traceRaysMulti(k.pts, np.broadcast_to(DIRS[j], (n, 3)), np.inf, k=0, count_all=True,
                                   counters=True)["counters"]
        multi += [int(c[0]), int(c[1])]
        if j == 0:
            multi1 = multi.copy()
    for v3 in (False, True):
        res = k.scene.signedDistance(k.pts, vote3=v3, votes=True, counters=True)
        assert_signed(res, k.exps[v3], True, f"counting kernel, vote3={v3}")
        plain = k.scene.signedDistance(k.pts, vote3=v3, votes=True)
        for key in ("t", "u", "v"):
            assert np.array_equal(bits(plain[key]), bits(res[key])), key
        assert np.array_equal(plain["tri_id"], res["tri_id"]) and np.array_equal(plain["votes"], res["votes"])
        c = [int(x) for x in res["counters"]]
        assert c[0] == int(ref[0]) and c[1] == int(ref[1])  # phase 1 is closestPoints' traversal
        # phase 2 reaches the multi-hit query's node records and leaves (the bound is +inf in both)
        assert (c[2], c[3]) == tuple((multi if v3 else multi1).tolist())
        print(f"suzanne, {n} points, vote3={v3}: nearest {c[0] / n:.1f} node records, {c[1] / n:.1f} triangle "
              f"evaluations; parity {c[2] / n:.1f} node records, {c[3] / n:.1f} triangle tests per point")
        cnt = np.zeros(4, np.uint64)  # occupancy mode: no nearest phase
        dev = torch.device("cuda", ctx.device)
        packed = np.zeros((n, 4), F)
        packed[:, 0:3], packed[:, 3] = k.pts, np.inf
        p_dev, out = torch.from_numpy(packed).to(dev), torch.empty((n,), dtype=torch.uint8, device=dev)
        torch.cuda.synchronize()
        assert k.scene.signedDistancesDevice(p_dev, n, out, mode=_lib.SIGNED_OCCUPANCY,
                                             flags=_lib.SIGNED_VOTE3 if v3 else 0, counters=cnt) == 0
        assert [int(x) for x in cnt] == [0, 0, c[2], c[3]]
        assert np.array_equal(out.cpu().numpy(), k.exps[v3]["inside"])


# ---- 10. chaining on the device ------------------------------------------------------------------------------------
def test_torch_chain_on_one_stream(ctx):
    import torch
    k = case(ctx, "suzanne")
    dev = torch.device("cuda", 0)
    tctx = beam.Context(device=0, stream=torch.cuda.current_stream(dev).cuda_stream)
    scene, keep = build(tctx, k.meshes)
    n = 800
    p = torch.from_numpy(np.ascontiguousarray(k.pts[:n])).to(dev)
    # no synchronisation from here to the end of the chain
    res = scene.signedDistance(p, vote3=True, votes=True)
    assert res["hits"].is_cuda and res["hits"].shape == (n, 4) and res["tri_id"].dtype == torch.int32
    assert res["votes"].dtype == torch.uint8 and res["votes"].shape == (n,)
    (pos,) = scene.hitAttributes(res["hits"], [(POS, 3)])
    gap = torch.linalg.vector_norm(p.double() - pos.double(), dim=1)
    packed = torch.cat([p, res["t"].abs()[:, None] * 0.5], dim=1).contiguous()  # the first result bounds a second query
    halfway = scene.signedDistance(packed, vote3=True)
    occ = scene.occupancy(p, vote3=True, votes=True)
    torch.cuda.synchronize()
    hits = res["hits"].cpu().numpy()
    exp = take(k.exps[True], np.arange(n))
    got = {"t": hits[:, 0], "u": hits[:, 1], "v": hits[:, 2], "tri_id": hits.view(np.uint32)[:, 3],
           "votes": res["votes"].cpu().numpy()}
    assert_signed(got, exp, True, "torch path")
    assert occ["inside"].dtype == torch.bool
    assert np.array_equal(occ["inside"].cpu().numpy(), exp["inside"].astype(bool))
    assert np.array_equal(occ["votes"].cpu().numpy(), exp["votes"])
    assert_rows(pos.cpu().numpy(), expected(k.meshes, hits, POS, 3), "closest point")
    # nothing within half the distance: the miss record, with the first query's sign
    h2 = halfway["hits"].cpu().numpy()
    off = np.abs(exp["t"]) > 0
    assert np.isinf(h2[off, 0]).all() and np.array_equal(np.signbit(h2[off, 0]), np.signbit(exp["t"][off]))
    scale = float(np.abs(k.pts[:n]).max() + np.abs(k.verts).max())
    assert np.abs(gap.cpu().numpy() - np.abs(exp["t"]).astype(np.float64)).max() <= 64 * 2.0 ** -24 * scale
    scene.destroy()
    tctx.close()


# ---- 11. errors --------------------------------------------------------------------------------------------------
def test_errors(ctx):
    import torch
    k = case(ctx, "suzanne")
    dev = torch.device("cuda", ctx.device)
    n = 64
    pts = torch.zeros((n + 1, 4), dtype=torch.float32, device=dev)
    out = torch.zeros((n + 1, 4), dtype=torch.float32, device=dev)
    votes = torch.zeros((n + 1,), dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    pp, op, vp = pts.data_ptr(), out.data_ptr(), votes.data_ptr()
    bad = _lib.ERROR_INVALID_PARAMETER
    unbuilt = beam.IScene.create(ctx)
    assert unbuilt.signedDistancesDevice(pp, n, op) == _lib.ERROR_NOT_BUILT
    unbuilt.destroy()
    s = k.scene
    cnt = np.zeros(4, np.uint64)
    for mode in (_lib.SIGNED_DISTANCE, _lib.SIGNED_OCCUPANCY):
        for flags in (0, _lib.SIGNED_VOTE3):
            assert s.signedDistancesDevice(pp, n, op, mode=mode, flags=flags) == 0
            assert s.signedDistancesDevice(pp, n, op, mode=mode, flags=flags, votes=vp + 1) == 0  # any alignment
            assert s.signedDistancesDevice(0, n, op, mode=mode, flags=flags) == bad
            assert s.signedDistancesDevice(pp, n, 0, mode=mode, flags=flags) == bad
            assert s.signedDistancesDevice(0, 0, 0, mode=mode, flags=flags) == 0  # n = 0: nothing to read or write
            off_p, off_o = pts.view(-1)[1:].data_ptr(), out.view(-1)[1:].data_ptr()  # 4 bytes in
            assert off_p == pp + 4 and off_o == op + 4
            assert s.signedDistancesDevice(off_p, n, op, mode=mode, flags=flags) == bad
            assert s.signedDistancesDevice(pp, n, off_o, mode=mode, flags=flags) == bad
        for flags in (2, 0x10, 0x80, 0x80000001):
            assert s.signedDistancesDevice(pp, n, op, mode=mode, flags=flags) == bad
            assert s.signedDistancesDevice(pp, n, op, mode=mode, flags=flags, counters=cnt) == bad
    for mode in (2, 3, 0xFFFFFFFF):
        assert s.signedDistancesDevice(pp, n, op, mode=mode) == bad
        assert s.signedDistancesDevice(pp, n, op, mode=mode, counters=cnt) == bad
    assert s.ctx.lib.bm_scene_signed_distances_counters(s.h, pp, n, 0, 0, op, None, None) == bad
    ctx.sync()
    tiny = [{"pos": F([[0, 0, 1], [1, 0, 1], [0, 1, 1]]), "nrm": F([[0, 0, 1]] * 3), "idx": np.uint32([0, 1, 2])}]
    for kw in ({"reference_kd": True}, {"reference_hash": True}, {"bvh_width": 2}):  # BVH8 contexts exist in A/B builds only
        other = beam.Context(device=0, **kw)
        sc, keep = build(other, tiny)
        assert sc.signedDistancesDevice(pp, n, op) == bad, kw
        assert sc.signedDistancesDevice(pp, n, op, counters=cnt) == bad, kw
        sc.destroy()
        other.close()
    with pytest.raises(beam.BeamError):
        s.sdfGrid((0, 0, 0), (1, 1, 1), (4, 0, 4))
    with pytest.raises(beam.BeamError):
        s.signedDistance(torch.zeros((4, 5), dtype=torch.float32, device=dev))


def test_repeated_device_context_queries_on_the_root(ctx):
    k = case(ctx, "suzanne")
    multi = beam.Context(devices=[0, 0])
    scene, keep = build(multi, k.meshes)
    check(scene, k.pts, np.inf, k.verts, "devices=[0, 0]", k.exps, cross=False)
    scene.destroy()
    multi.close()
