"""GPU checks of sphere-cast queries (bm_scene_sweep_spheres).

The yardstick is tests/test_sweep_abi.py: the numpy float32 restatement of the header's swept-sphere function,
evaluated over ALL triangles, the lexicographic minimum of (t, id). The traversal prunes, the brute force does
not; t, u, v (as bit images), tri_id and the any byte must be equal. No expected value comes from the library.
"""
from types import SimpleNamespace

import numpy as np
import pytest

import deep_scenes
from raytracercuda_amd import _lib, beam, scenes
from test_gpu_attrs import assert_rows, expected
from test_gpu_points import bits, build, soup, take, tri_vertices
from test_instances_abi import MIRROR, rotation, xform_mesh
from test_points_abi import tri_nearest
from test_sweep_abi import (COVER, COVER_TRI, NO_TRI, SHIFT, START, bounds, brute_force_sweep, cover_sweeps,
                            make_sweeps, translated)

pytestmark = pytest.mark.gpu

F = np.float32
MISS = np.uint32(NO_TRI)
QUAD_LDS = 24  # stack entries a query keeps in LDS (bm_trace_quad.h); beyond: the global overflow area
POS, FACE = beam.VERTEX_DATA_POSITION, beam.ATTR_MESH_FACE
# | |c(t) - position| - r | of the GPU's interpolated contact against the float64 value of the same expression from
# the restatement's record, in units of 2^-24 * S (S: the largest |coordinate| of origin, centre and mesh).
# Measured on an MI355X: 0.54 after the refit, 0.73 with instances; asserted at 4 x that, rounded up to a power of two.
CHAIN_MEASURED = 0.73
CHAIN_TOL = 4.0


def assert_records(res, exp, where=None, what=""):
    sel = slice(None) if where is None else where
    bad = res["tri_id"][sel] != exp["tri_id"][sel]
    assert not bad.any(), f"{what}: tri_id differs on {int(bad.sum())} sweeps, first {np.flatnonzero(bad)[:5]}"
    for k in ("t", "u", "v"):
        diff = bits(res[k][sel]) != bits(exp[k][sel])
        assert not diff.any(), f"{what}: {k} differs on {int(diff.sum())} sweeps, first {np.flatnonzero(diff)[:5]}"


def check(scene, sweeps, verts, what, exp=None):
    """Both modes of the query over sweeps = (o, d, r, tmax) against the brute force; returns it."""
    exp = brute_force_sweep(*sweeps, verts) if exp is None else exp
    assert_records(scene.sweepSpheres(*sweeps), exp, what=what)
    got = scene.sweepSpheres(*sweeps, any=True)["any"]
    assert np.array_equal(got, exp["any"].astype(bool)), f"{what}: any byte differs on {int((got != exp['any']).sum())}"
    return exp


def mixed_sweeps(verts, n, seed):
    """make_sweeps with half the radii 0.2-30 % of the diagonal, a quarter 1e-5-1e-4 and a quarter 1e-3-1e-2."""
    half, quarter = n // 2, n // 4
    parts = [make_sweeps(verts, half, seed), make_sweeps(verts, quarter, seed + 1, (1e-5, 1e-4)),
             make_sweeps(verts, n - half - quarter, seed + 2, (1e-3, 1e-2))]
    return tuple(np.concatenate([p[k] for p in parts]) for k in range(4))


_CASES = {}


def case(ctx, name, n=3904):
    """Mesh, GPU scene, the sweeps and the brute force's answers for them — computed once per module run."""
    if name not in _CASES:
        meshes = scenes.load_mesh(name)
        scene, keep = build(ctx, meshes)
        verts = tri_vertices(meshes)
        sw = mixed_sweeps(verts, n, 7)
        exp = brute_force_sweep(*sw, verts)
        _CASES[name] = SimpleNamespace(meshes=meshes, scene=scene, keep=keep, sw=sw, verts=verts, exp=exp)
    return _CASES[name]


def teardown_module(module):
    for k in _CASES.values():
        k.scene.destroy()
    _CASES.clear()


def sub(sw, sel):
    return tuple(a[sel] for a in sw)


# ---- 1. one triangle: every candidate ----------------------------------------------------------------
def test_one_triangle_every_candidate(ctx):
    scene, keep = build(ctx, soup(COVER_TRI))
    exp = check(scene, cover_sweeps(), COVER_TRI, "designed sweeps")
    assert exp["kind"].tolist() == [c[2] for c in COVER]
    rng = np.random.default_rng(3)
    o = F(rng.uniform(-3, 3, (400, 3)))
    d = F(rng.uniform(-0.5, 2.5, (400, 3)) * [1, 1, 0]) - o  # towards points in and around the triangle
    r = F(np.exp(rng.uniform(np.log(1e-3), np.log(1.0), 400)))
    exp = check(scene, (o, d, r, np.full(400, np.inf, F)), COVER_TRI, "random sweeps")
    assert set(exp["kind"].tolist()) >= set(range(8)), sorted(set(exp["kind"].tolist()))
    scene.destroy()


# ---- 2. small scenes -----------------------------------------------------------------------------------
@pytest.mark.parametrize("ntri", [0, 2, 4, 5, 17])
def test_small_scenes(ctx, ntri):
    rng = np.random.default_rng(300 + ntri)
    base = rng.uniform(-1, 1, (ntri, 1, 3))
    verts = F(base + rng.uniform(-0.4, 0.4, (ntri, 3, 3)))
    scene, keep = build(ctx, soup(verts) if ntri else [])
    o = F(rng.uniform(-3, 3, (203, 3)))
    d = F(rng.uniform(-1, 1, (203, 3))) - o
    r = F(rng.uniform(0.05, 0.5, 203))
    sw = (o, d, r, np.full(203, np.inf, F))
    if ntri == 0:  # a built scene with no triangles: all misses
        res = scene.sweepSpheres(*sw)
        assert (res["tri_id"] == MISS).all() and np.isposinf(res["t"]).all()
        assert (bits(res["u"]) == 0).all() and (bits(res["v"]) == 0).all()
        assert not scene.sweepSpheres(*sw, any=True)["any"].any()
    else:
        exp = check(scene, sw, verts, f"{ntri} triangles")
        assert 20 < (exp["tri_id"] != MISS).sum() < 203
    scene.destroy()


# ---- 3. meshes -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,n", [("suzanne", 3904), ("bunny", 1001)])
def test_meshes_against_brute_force(ctx, name, n):
    k = case(ctx, name, n)
    assert k.sw[0].shape[0] == n
    hit = k.exp["tri_id"] != MISS
    assert 0.4 * n < hit.sum() < n and len(set(k.exp["tri_id"][hit].tolist())) > 100
    assert (k.exp["kind"] == START).sum() >= 0.01 * n
    check(k.scene, k.sw, k.verts, name, k.exp)


def test_translated_suzanne(ctx):
    moved = translated(scenes.load_mesh("suzanne"), SHIFT)
    verts = tri_vertices(moved)
    sw = mixed_sweeps(verts, 1302, 17)
    scene, keep = build(ctx, moved)
    exp = check(scene, sw, verts, "translated suzanne")
    assert (exp["tri_id"] != MISS).sum() > 500
    scene.destroy()


# ---- 4. ties -------------------------------------------------------------------------------------------
def test_ties_resolve_to_the_lowest_id(ctx):
    k = case(ctx, "suzanne")
    scene, keep = build(ctx, k.meshes + k.meshes)  # the same mesh as two plain entries
    sel = np.arange(0, k.sw[0].shape[0], 6)
    res = scene.sweepSpheres(*sub(k.sw, sel))
    hit = res["tri_id"] != MISS
    assert (res["tri_id"][hit] < k.verts.shape[0]).all()
    assert_records(res, take(k.exp, sel), what="mesh added twice")  # the copy never wins: the single mesh's answers
    scene.destroy()


# ---- 5. shared edges and vertices ----------------------------------------------------------------------
def test_shared_edges_and_vertices_stop_the_sphere(ctx):
    g = 5  # a unit quad of 4 x 4 cells, two triangles each
    x, y = np.meshgrid(np.arange(g) / (g - 1), np.arange(g) / (g - 1), indexing="ij")
    p = np.stack([x, y, np.zeros_like(x)], axis=2)
    tris = []
    for i in range(g - 1):
        for j in range(g - 1):
            tris += [[p[i, j], p[i + 1, j], p[i + 1, j + 1]], [p[i, j], p[i + 1, j + 1], p[i, j + 1]]]
    verts = F(tris)
    rng = np.random.default_rng(8)
    inner = p[1:-1, 1:-1].reshape(-1, 3)                                   # shared vertices
    mids = np.concatenate([(p[1:-1, :-1] + p[1:-1, 1:]).reshape(-1, 3) / 2,  # the middle of shared edges
                           (p[:-1, 1:-1] + p[1:, 1:-1]).reshape(-1, 3) / 2,
                           (p[:-1, :-1] + p[1:, 1:]).reshape(-1, 3) / 2])    # and of the cells' diagonals
    targets = np.concatenate([inner, mids])
    targets = np.tile(targets, (4, 1))
    o = F(targets + rng.uniform(-1, 1, targets.shape) * [1, 1, 0] + [0, 0, 1] * rng.choice([-2.0, 0.5, 3.0], (targets.shape[0], 1)))
    d = F(targets) - o
    sw = (o, d, np.full(o.shape[0], 0.01, F), np.full(o.shape[0], np.inf, F))
    scene, keep = build(ctx, soup(verts))
    exp = check(scene, sw, verts, "tessellated quad")
    assert (exp["tri_id"] != MISS).all()  # no sweep passes through
    assert ((exp["t"] > 0.9) & (exp["t"] < 1.0)).all()  # and each stops one radius short of its target
    scene.destroy()


# ---- 6. start overlap ----------------------------------------------------------------------------------
def test_start_overlap_gives_t_zero_with_the_nearest_points_uv(ctx):
    k = case(ctx, "suzanne")
    rng = np.random.default_rng(12)
    n = 600
    f = rng.integers(0, k.verts.shape[0], n)
    w = rng.dirichlet([1, 1, 1], n)
    on = (k.verts[f].astype(np.float64) * w[:, :, None]).sum(axis=1)
    r = F(rng.uniform(0.01, 0.1, n))
    o = F(on + rng.normal(size=(n, 3)) * 0.3 * r[:, None])  # within r of the surface
    d = F(rng.normal(size=(n, 3)))
    tmax = np.where(np.arange(n) % 3 == 0, F(0.0), F(np.inf)).astype(F)
    exp = check(k.scene, (o, d, r, tmax), k.verts, "start overlap")
    assert (exp["kind"] == START).all() and (exp["t"] == 0).all()
    g = exp["tri_id"]
    dd, u, v, _ = tri_nearest(o, k.verts[g, 0], k.verts[g, 1], k.verts[g, 2])
    assert np.array_equal(bits(u), bits(exp["u"])) and np.array_equal(bits(v), bits(exp["v"]))
    away = (o + F(10) * F([1, 0, 0]), d, r, np.zeros(n, F))  # tmax = 0 away from the surface: nothing
    assert (check(k.scene, away, k.verts, "tmax = 0, no overlap")["tri_id"] == MISS).all()


# ---- 7. tmax -------------------------------------------------------------------------------------------
def test_tmax_bounds_the_result(ctx):
    k = case(ctx, "suzanne")
    sel = np.flatnonzero(np.isposinf(k.sw[3]))[::8]
    o, d, r, _ = sub(k.sw, sel)
    t = k.exp["t"][sel]
    tmax = np.concatenate([t, np.nextafter(t, F(0)), t * F(0.5)])
    tmax = np.where(np.isfinite(tmax), tmax, F(3.0)).astype(F)  # the misses: some bound
    sw = (np.tile(o, (3, 1)), np.tile(d, (3, 1)), np.tile(r, 3), tmax)
    exp = check(k.scene, sw, k.verts, "tmax")
    m = sel.size
    moving = (k.exp["tri_id"][sel] != MISS) & (t > 0)
    assert moving.sum() > m // 3
    assert_records(take(exp, np.arange(m)), take(k.exp, sel), where=moving, what="tmax = t keeps the contact")
    assert (exp["t"][m:2 * m][moving] != t[moving]).all()  # one ulp below: that contact is out of reach


# ---- 8. direction scale ------------------------------------------------------------------------------
def test_direction_scale(ctx):
    k = case(ctx, "suzanne")
    sel = np.arange(0, k.sw[0].shape[0], 8)
    o, d, r, tmax = sub(k.sw, sel)
    for s in (0.5, 2.0):
        exp = check(k.scene, (o, d * F(s), r, tmax / F(s)), k.verts, f"dir x {s}")
        both = (exp["tri_id"] != MISS) & (k.exp["tri_id"][sel] != MISS)
        assert both.sum() > sel.size // 3
        rel = np.abs(exp["t"][both] * F(s) - k.exp["t"][sel][both]) / np.maximum(k.exp["t"][sel][both], F(1e-30))
        assert np.median(rel) < 1e-6  # t scales; the equality is with the restatement, not with this rule


# ---- 9. axis-aligned directions ----------------------------------------------------------------------
def test_axis_aligned_directions(ctx):
    k = case(ctx, "suzanne")
    rec, _, _, _ = k.scene.export()
    box = rec[:, :24].view(F).reshape(-1, 6, 4)
    planes = box[:64].transpose(0, 2, 1).reshape(-1, 6)
    planes = planes[np.isfinite(planes).all(axis=1)][:96]  # child boxes of the top records
    lo, hi = bounds(k.verts)
    rng = np.random.default_rng(4)
    o, d = [], []
    for j, b in enumerate(planes):
        axis, travel = j % 3, (j // 3) % 3
        if travel == axis:
            travel = (axis + 1) % 3
        p = rng.uniform(lo, hi)
        p[axis] = b[axis + 3 * (j % 2)]            # on a box plane of this axis
        p[travel] = lo[travel] - 0.5 if j % 4 < 2 else hi[travel] + 0.5
        e = np.zeros(3)
        e[travel] = 1.0 if j % 4 < 2 else -1.0     # along one axis: two zero components
        if j % 5 == 0:
            e[3 - axis - travel] = 0.25            # or one
        o.append(p)
        d.append(e)
    o, d = F(o), F(d)
    d[::7] = np.where(d[::7] == 0, F(-0.0), d[::7])  # a negative zero is a zero
    r = F(rng.choice([1e-4, 0.02, 0.3], o.shape[0]))
    exp = check(k.scene, (o, d, r, np.full(o.shape[0], np.inf, F)), k.verts, "axis-aligned")
    assert 10 < (exp["tri_id"] != MISS).sum() < o.shape[0]


# ---- 10. any-mode ------------------------------------------------------------------------------------
def test_any_mode_equals_the_closest_modes_reach(ctx):
    k = case(ctx, "suzanne")
    closest = k.scene.sweepSpheres(*k.sw)
    any_ = k.scene.sweepSpheres(*k.sw, any=True)["any"]
    assert any_.dtype == bool and np.array_equal(any_, (closest["t"] <= k.sw[3]) & np.isfinite(closest["t"]))
    assert 0 < any_.sum() < any_.size


# ---- 11. invalid sweeps ------------------------------------------------------------------------------
def test_invalid_sweeps_get_the_miss_record(ctx):
    k = case(ctx, "suzanne")
    n = 660
    o, d, r, tmax = (a[:n].copy() for a in k.sw)
    sel = np.arange(3, n, 5)
    kind = (sel // 5) % 13
    for c in range(3):
        o[sel[kind == c], c] = np.nan
        d[sel[kind == 3 + c], c] = np.inf if c != 1 else -np.inf
    d[sel[kind == 6]] = 0.0
    d[sel[kind == 7]] = F([0.0, -0.0, 0.0])
    tmax[sel[kind == 8]] = np.nan
    tmax[sel[kind == 9]] = -1.0
    r[sel[kind == 10]] = 0.0
    r[sel[kind == 11]] = -0.5
    r[sel[kind == 12]] = np.where(np.arange((kind == 12).sum()) % 2 == 0, np.nan, np.inf)
    invalid = np.zeros(n, bool)
    invalid[sel] = True
    assert all((kind == j).sum() >= 5 for j in range(13))
    exp = brute_force_sweep(o, d, r, tmax, k.verts)
    assert (exp["tri_id"][invalid] == MISS).all() and not exp["any"][invalid].any()
    assert_records(exp, take(k.exp, np.arange(n)), ~invalid, "the yardstick's neighbours")
    res = k.scene.sweepSpheres(o, d, r, tmax, counters=True)
    assert_records(res, exp, what="with invalid sweeps")
    assert (bits(res["u"][invalid]) == 0).all() and (bits(res["v"][invalid]) == 0).all()
    assert np.isposinf(res["t"][invalid]).all()
    assert int(res["counters"][2]) == int((exp["tri_id"] != MISS).sum())
    assert np.array_equal(k.scene.sweepSpheres(o, d, r, tmax, any=True)["any"], exp["any"].astype(bool))
    for flag in (False, True):
        alone = k.scene.sweepSpheres(o[invalid], d[invalid], r[invalid], tmax[invalid], any=flag, counters=True)
        assert [int(x) for x in alone["counters"]] == [0, 0, 0, 0]  # invalid sweeps count nothing


# ---- 12. batch edges ---------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 15, 16, 17, 63, 64, 65])
def test_batch_edges_write_nothing_past_n(ctx, n):
    import torch
    k = case(ctx, "suzanne")
    dev = torch.device("cuda", ctx.device)
    packed = np.zeros((n, 8), F)
    packed[:, 0:3], packed[:, 3], packed[:, 4:7], packed[:, 7] = k.sw[0][:n], k.sw[3][:n], k.sw[1][:n], k.sw[2][:n]
    hits = torch.full((n + 64, 4), -7.5, dtype=torch.float32, device=dev)
    flags = torch.full((n + 256,), 77, dtype=torch.uint8, device=dev)
    s_dev = torch.from_numpy(packed).to(dev)
    torch.cuda.synchronize()
    assert k.scene.sweepSpheresDevice(s_dev.data_ptr(), n, hits.data_ptr()) == 0
    assert k.scene.sweepSpheresDevice(s_dev, n, flags, mode=_lib.SWEEP_ANY) == 0  # tensors serve as pointers
    ctx.sync()
    h, a = hits.cpu().numpy(), flags.cpu().numpy()
    assert np.all(h[n:] == F(-7.5)) and np.all(a[n:] == 77)
    got = {"t": h[:n, 0], "u": h[:n, 1], "v": h[:n, 2], "tri_id": h.view(np.uint32)[:n, 3]}
    assert_records(got, take(k.exp, np.arange(n)), what=f"n = {n}")
    assert np.array_equal(a[:n], k.exp["any"][:n])


@pytest.mark.parametrize("grid", [1, 2])
def test_small_grid_strides_over_the_batches(ctx, grid):
    k = case(ctx, "suzanne")
    small = beam.Context(device=0, params={"trace_grid": grid})
    scene, keep = build(small, k.meshes)
    sel = np.arange(0, 1500)
    check(scene, sub(k.sw, sel), k.verts, f"trace_grid {grid}", take(k.exp, sel))
    scene.destroy()
    small.close()


# ---- 13. the stack's overflow area ---------------------------------------------------------------------
def test_deep_chain_uses_the_overflow_area(ctx):
    meshes = deep_scenes.deep_meshes()
    verts = tri_vertices(meshes)
    o, d = deep_scenes.ray_batch(480)
    r = np.full(480, 64.0, F)  # the sphere meets the boxes of the chain's siblings
    sw = (o, d, r, np.full(480, np.inf, F))
    exp = brute_force_sweep(*sw, verts)
    assert (exp["tri_id"] != MISS).sum() > 100
    scene, keep = build(ctx, meshes)
    res = scene.sweepSpheres(*sw, counters=True)
    deepest = int(res["counters"][3])
    print(f"deep chain: {verts.shape[0]} triangles, deepest stack {deepest} entries (LDS holds {QUAD_LDS})")
    assert deepest >= 25, f"the overflow path did not run: deepest stack {deepest}"
    assert_records(res, exp, what="deep chain, counting kernel")
    check(scene, sw, verts, "deep chain", exp)
    scene.destroy()


# ---- 14. counters --------------------------------------------------------------------------------------
def test_counters(ctx):
    k = case(ctx, "suzanne")
    n = k.sw[0].shape[0]
    scene = k.scene
    rec, _, _, _ = scene.export()
    seen, front = 0, np.zeros(1, np.int64)
    while front.size:  # the records a traversal can reach: what an exhaustive walk fetches
        seen += front.size
        ref = rec[front, 24:28].reshape(-1)
        front = ref[(ref != 0xFFFFFFFF) & ((ref & 0x80000000) == 0)].astype(np.int64)
    res = scene.sweepSpheres(*k.sw, counters=True)
    assert_records(res, k.exp, what="counting kernel")
    plain = scene.sweepSpheres(*k.sw)
    for key in ("t", "u", "v", "tri_id"):
        assert np.array_equal(bits(plain[key]) if key != "tri_id" else plain[key],
                              bits(res[key]) if key != "tri_id" else res[key]), key
    nodes, tris, found, deepest = (int(x) for x in res["counters"])
    records = seen
    print(f"suzanne, {n} sweeps: {nodes / n:.1f} of {records} node records and {tris / n:.1f} triangle evaluations "
          f"per sweep, deepest stack {deepest}")
    assert found == int((k.exp["tri_id"] != MISS).sum())
    assert 0 < nodes < 0.05 * n * records, (nodes, n * records)  # an exhaustive walk fetches every record
    assert deepest > 0
    anyc = scene.sweepSpheres(*k.sw, any=True, counters=True)
    assert np.array_equal(anyc["any"], k.exp["any"].astype(bool))
    assert int(anyc["counters"][2]) == int(k.exp["any"].sum()) and int(anyc["counters"][0]) <= nodes


# ---- 15. refit, instances and hit attributes ---------------------------------------------------------
def chain_error(scene, meshes, sw, exp, what):
    """The query chained into hitAttributes: the rows equal the attribute yardstick's, and | |c(t) - position| - r |
    of the GPU's position against the float64 value of the same expression from the restatement's record."""
    res = scene.sweepSpheres(*sw)
    assert_records(res, exp, what=what)
    n = sw[0].shape[0]
    hits = np.zeros((n, 4), F)
    hits[:, 0], hits[:, 1], hits[:, 2] = res["t"], res["u"], res["v"]
    hits.view(np.uint32)[:, 3] = res["tri_id"]
    pos, face = scene.hitAttributes(hits, [(POS, 3), (FACE, 2)])
    assert_rows(pos, expected(meshes, hits, POS, 3), what + ": contact point")
    assert_rows(face, expected(meshes, hits, FACE, 2), what + ": owner")
    hit = exp["tri_id"] != MISS
    verts = tri_vertices(meshes).astype(np.float64)
    o, d, r = (a[hit].astype(np.float64) for a in sw[:3])
    t, u, v = (exp[key][hit].astype(np.float64) for key in ("t", "u", "v"))
    tv = verts[exp["tri_id"][hit]]
    centre = o + t[:, None] * d
    ref = tv[:, 0] * (1 - (u + v))[:, None] + tv[:, 1] * u[:, None] + tv[:, 2] * v[:, None]
    e_ref = np.abs(np.linalg.norm(centre - ref, axis=1) - r)
    e_gpu = np.abs(np.linalg.norm(centre - pos[hit].astype(np.float64), axis=1) - r)
    S = np.maximum(np.maximum(np.abs(o).max(axis=1), np.abs(centre).max(axis=1)), np.abs(verts).max())
    worst = float((np.abs(e_gpu - e_ref) / (2.0 ** -24 * S)).max())
    print(f"{what}: largest difference of | |c(t) - position| - r | from its float64 value {worst:.2f} x 2^-24 S "
          f"over {int(hit.sum())} contacts")
    assert hit.sum() > n // 3
    assert worst <= CHAIN_TOL, worst
    return face


def test_after_refit_chained_into_hit_attributes(ctx):
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
    verts = tri_vertices(moved)
    sw = mixed_sweeps(verts, 900, 21)
    chain_error(scene, moved, sw, brute_force_sweep(*sw, verts), "after refit")
    scene.destroy()


def test_instances_chained_into_hit_attributes(ctx):
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
    verts = tri_vertices(pre)
    sw = mixed_sweeps(verts, 900, 33)
    exp = brute_force_sweep(*sw, verts)
    ntri = k.verts.shape[0]
    hit = exp["tri_id"] != MISS
    assert set((exp["tri_id"][hit] // ntri).tolist()) == {0, 1, 2}
    face = chain_error(scene, pre, sw, exp, "instances")
    assert np.array_equal(face[hit, 0], (exp["tri_id"][hit] // ntri).astype(np.int32))  # m is the entry index
    scene.destroy()


# ---- 16. chaining on the device ------------------------------------------------------------------------
def test_torch_chain_on_one_stream(ctx):
    import torch
    k = case(ctx, "suzanne")
    dev = torch.device("cuda", 0)
    tctx = beam.Context(device=0, stream=torch.cuda.current_stream(dev).cuda_stream)
    scene, keep = build(tctx, k.meshes)
    n = 1500
    o, d, r, tmax = (torch.from_numpy(np.ascontiguousarray(a[:n])).to(dev) for a in k.sw)
    # no synchronisation from here to the end of the chain
    res = scene.sweepSpheres(o, d, r, tmax)
    assert res["hits"].is_cuda and res["hits"].shape == (n, 4) and res["tri_id"].dtype == torch.int32
    (pos,) = scene.hitAttributes(res["hits"], [(POS, 3)])
    centre = o.double() + res["t"].double()[:, None] * d.double()
    gap = torch.linalg.vector_norm(centre - pos.double(), dim=1)
    packed = torch.cat([o, tmax[:, None], d, r[:, None]], dim=1).contiguous()
    again = scene.sweepSpheres(packed)
    reach = scene.sweepSpheres(packed, any=True)
    halfway = scene.sweepSpheres(o, d, r, res["t"] * 0.5, any=True)  # the first query's result bounds a second one
    torch.cuda.synchronize()
    hits = res["hits"].cpu().numpy()
    got = {"t": hits[:, 0], "u": hits[:, 1], "v": hits[:, 2], "tri_id": hits.view(np.uint32)[:, 3]}
    exp = take(k.exp, np.arange(n))
    assert_records(got, exp, what="torch path")
    assert torch.equal(again["hits"].view(torch.int32), res["hits"].view(torch.int32))
    assert np.array_equal(reach["any"].cpu().numpy(), exp["any"].astype(bool))
    assert_rows(pos.cpu().numpy(), expected(k.meshes, hits, POS, 3), "contact point")
    moving = (exp["tri_id"] != MISS) & (exp["t"] > 0)
    assert not halfway["any"].cpu().numpy()[moving & np.isfinite(exp["t"])].any()  # nothing within half the way
    # the contact lies one radius from the centre: within the function's own error (test_sweep_abi.QUALITY)
    err = np.abs(gap.cpu().numpy() - k.sw[2][:n].astype(np.float64))[moving]
    scale = float(np.abs(k.sw[0][:n]).max() + np.abs(k.verts).max())
    assert err.max() <= 65536 * 2.0 ** -24 * scale
    scene.destroy()
    tctx.close()


# ---- 17. errors ----------------------------------------------------------------------------------------
def test_errors(ctx):
    import torch
    k = case(ctx, "suzanne")
    dev = torch.device("cuda", ctx.device)
    n = 64
    sw = torch.zeros((n + 1, 8), dtype=torch.float32, device=dev)
    out = torch.zeros((n + 1, 4), dtype=torch.float32, device=dev)
    torch.cuda.synchronize()
    sp, op = sw.data_ptr(), out.data_ptr()
    bad = _lib.ERROR_INVALID_PARAMETER
    unbuilt = beam.IScene.create(ctx)
    assert unbuilt.sweepSpheresDevice(sp, n, op) == _lib.ERROR_NOT_BUILT
    unbuilt.destroy()
    s = k.scene
    cnt = np.zeros(4, np.uint64)
    for mode in (_lib.SWEEP_CLOSEST, _lib.SWEEP_ANY):
        assert s.sweepSpheresDevice(sp, n, op, mode=mode) == 0
        assert s.sweepSpheresDevice(0, n, op, mode=mode) == bad and s.sweepSpheresDevice(sp, n, 0, mode=mode) == bad
        assert s.sweepSpheresDevice(0, 0, 0, mode=mode) == 0  # n = 0: nothing to read or write
        off_s, off_o = sw.view(-1)[1:].data_ptr(), out.view(-1)[1:].data_ptr()  # 4 bytes in
        assert off_s == sp + 4 and off_o == op + 4
        assert s.sweepSpheresDevice(off_s, n, op, mode=mode) == bad and s.sweepSpheresDevice(sp, n, off_o, mode=mode) == bad
        for flags in (1, 0x10, 0x80, 0x80000000):  # no flag bits are defined, the ray query's included
            assert s.sweepSpheresDevice(sp, n, op, mode=mode, flags=flags) == bad
            assert s.sweepSpheresDevice(sp, n, op, mode=mode, counters=cnt, flags=flags) == bad
    for mode in (2, 3, 0xFFFFFFFF):
        assert s.sweepSpheresDevice(sp, n, op, mode=mode) == bad
        assert s.sweepSpheresDevice(sp, n, op, mode=mode, counters=cnt) == bad
    assert s.ctx.lib.bm_scene_sweep_spheres_counters(s.h, sp, n, 0, 0, op, None) == bad
    ctx.sync()
    tiny = [{"pos": F([[0, 0, 1], [1, 0, 1], [0, 1, 1]]), "nrm": F([[0, 0, 1]] * 3), "idx": np.uint32([0, 1, 2])}]
    for kw in ({"reference_kd": True}, {"reference_hash": True}, {"bvh_width": 2}):  # BVH8 contexts exist in A/B builds only
        other = beam.Context(device=0, **kw)
        sc, keep = build(other, tiny)
        assert sc.sweepSpheresDevice(sp, n, op) == bad, kw
        assert sc.sweepSpheresDevice(sp, n, op, counters=cnt) == bad, kw
        sc.destroy()
        other.close()


def test_repeated_device_context_queries_on_the_root(ctx):
    k = case(ctx, "suzanne")
    multi = beam.Context(devices=[0, 0])
    scene, keep = build(multi, k.meshes)
    sel = np.arange(0, 1500)
    check(scene, sub(k.sw, sel), k.verts, "devices=[0, 0]", take(k.exp, sel))
    scene.destroy()
    multi.close()
