"""GPU checks of hit attributes (bm_scene_hit_attributes): the meshes' vertex slots interpolated at hit records.

The expected values are a numpy float32 restatement of the header's formula, one operation per numpy
statement so that nothing fuses: w = 1 - (u + v); out = (a0*w + a1*u) + a2*v, the normalisation
v * (1 / sqrt((x*x + y*y) + z*z)) and the cross product of the geometric normal. Results are compared bit for
bit. The host's triangle -> (mesh, face) mapping is an enumeration, not a search. Hit records come from
IScene.traceRays (whose correctness is test_gpu_rays.py's business) or are made by hand.
"""
import ctypes as C
from types import SimpleNamespace

import numpy as np
import pytest

from raytracercuda_amd import _lib, beam, scenes

pytestmark = pytest.mark.gpu

F = np.float32
NO_TRI = 0xFFFFFFFF
GROUPS, PER = 64, 61  # 3,904 rays, the batch construction of test_gpu_rays.make_batch
POS, NRM, UV1, TAN, BIT = (beam.VERTEX_DATA_POSITION, beam.VERTEX_DATA_NORMAL, beam.VERTEX_DATA_UV1,
                           beam.VERTEX_DATA_TANGENT, beam.VERTEX_DATA_BITANGENT)
EX1, EX2, EX4 = beam.VERTEX_DATA_EXTRA1, beam.VERTEX_DATA_EXTRA2, beam.VERTEX_DATA_EXTRA4
GEOM, FACE, NORMALIZE = beam.ATTR_GEOM_NORMAL, beam.ATTR_MESH_FACE, beam.ATTR_NORMALIZE
BAD, FORMAT, NOT_BUILT = _lib.ERROR_INVALID_PARAMETER, _lib.ERROR_INVALID_FORMAT, _lib.ERROR_NOT_BUILT
# every request the Suzanne tests make: the four synthetic slots, position, normal and the pseudo-slots
SUZ_REQS = [(UV1, 2, 0), (EX1, 1, 0), (EX2, 4, 0), (TAN, 3, 0), (POS, 3, 0), (NRM, 3, 0), (GEOM, 3, 0), (FACE, 2, 0),
            (NRM, 3, NORMALIZE), (GEOM, 3, NORMALIZE), (TAN, 3, NORMALIZE)]


def bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


# ---- the restatement ---------------------------------------------------------------------------------
def interp(a0, a1, a2, u, v):
    """(a0*w + a1*u) + a2*v with w = 1 - (u + v): float32 arrays, one rounding per statement."""
    assert all(x.dtype == F for x in (a0, a1, a2, u, v))
    with np.errstate(all="ignore"):
        s = u + v
        w = F(1.0) - s
        p0 = a0 * w[:, None]
        p1 = a1 * u[:, None]
        q = p0 + p1
        p2 = a2 * v[:, None]
        return q + p2


def normalize(n):
    assert n.dtype == F and n.shape[1] == 3
    with np.errstate(all="ignore"):
        xx = n[:, 0] * n[:, 0]
        yy = n[:, 1] * n[:, 1]
        zz = n[:, 2] * n[:, 2]
        d = xx + yy
        d = d + zz
        r = np.sqrt(d)
        il = F(1.0) / r
        return n * il[:, None]


def geom_normal(v0, v1, v2):
    assert v0.dtype == F
    e1 = v1 - v0
    e2 = v2 - v0
    out = np.zeros_like(v0)
    for c, (i, j) in enumerate(((1, 2), (2, 0), (0, 1))):
        a = e1[:, i] * e2[:, j]
        b = e2[:, i] * e1[:, j]
        out[:, c] = a - b
    return out


def slot_data(m, slot):
    if slot == POS:
        return np.asarray(m["pos"], F).reshape(-1, 3)
    if slot == NRM:
        return np.asarray(m["nrm"], F).reshape(-1, 3)
    d = (m.get("slots") or {}).get(slot)
    return None if d is None else np.asarray(d, F)


def mapping(meshes):
    """Global triangle id -> (scene mesh index, face index), by enumeration."""
    counts = [np.asarray(m["idx"]).size // 3 for m in meshes]
    mesh_of = np.concatenate([np.full(c, i, np.int64) for i, c in enumerate(counts)] + [np.zeros(0, np.int64)])
    face_of = np.concatenate([np.arange(c, dtype=np.int64) for c in counts] + [np.zeros(0, np.int64)])
    return mesh_of, face_of


def records(t, u, v, tri):
    h = np.zeros((len(tri), 4), F)
    h[:, 0], h[:, 1], h[:, 2] = t, u, v
    h.view(np.uint32)[:, 3] = tri
    return h


def expected(meshes, hits, slot, comps, flags=0):
    """The rows bm_scene_hit_attributes must write for one request."""
    n = hits.shape[0]
    g = hits.view(np.uint32)[:, 3].astype(np.int64)
    u, v = np.ascontiguousarray(hits[:, 1]), np.ascontiguousarray(hits[:, 2])
    mesh_of, face_of = mapping(meshes)
    live = g < mesh_of.size
    gl = np.where(live, g, 0)
    if slot == FACE:
        out = np.full((n, 2), -1, np.int32)
        out[live, 0], out[live, 1] = mesh_of[gl[live]], face_of[gl[live]]
        return out
    out = np.zeros((n, comps), F)
    if mesh_of.size == 0:
        return out
    for i, m in enumerate(meshes):
        data = slot_data(m, POS if slot == GEOM else slot)
        sel = np.flatnonzero(live & (mesh_of[gl] == i))
        if data is None or sel.size == 0:
            continue
        assert slot == GEOM or data.shape[1] == comps
        iv = np.asarray(m["idx"]).reshape(-1, 3).astype(np.int64)[face_of[g[sel]]]
        a0, a1, a2 = data[iv[:, 0]], data[iv[:, 1]], data[iv[:, 2]]
        rows = geom_normal(a0, a1, a2) if slot == GEOM else interp(a0, a1, a2, u[sel], v[sel])
        out[sel] = normalize(rows) if flags & NORMALIZE else rows
    return out


def query(scene, hits, reqs):
    """hitAttributes over any number of requests, four per call."""
    out = []
    for k in range(0, len(reqs), beam.ATTR_MAX_REQS):
        out += scene.hitAttributes(hits, reqs[k:k + beam.ATTR_MAX_REQS])
    return out


def assert_rows(got, exp, what=""):
    assert got.shape == exp.shape and got.dtype == exp.dtype, (what, got.shape, exp.shape, got.dtype, exp.dtype)
    same = got.view(np.uint32) == exp.view(np.uint32)
    assert same.all(), f"{what}: {int((~same.all(axis=1)).sum())} of {got.shape[0]} rows differ"


def check(scene, meshes, hits, reqs):
    for r, got in zip(reqs, query(scene, hits, reqs)):
        r = tuple(r) + (0,) * (3 - len(r))
        assert_rows(got, expected(meshes, hits, *r), f"request {r}")


# ---- scenes ------------------------------------------------------------------------------------------
def build(ctx, meshes):
    scene = beam.IScene.create(ctx)
    keep = beam.upload_meshes(ctx, scene, meshes)
    scene.updateGPUScene()
    return scene, keep


def with_slots(meshes, seed, skip_uv=()):
    """The meshes with synthetic UV1 (2 components), EXTRA1 (1), EXTRA2 (4) and TANGENT (3) slots."""
    rng = np.random.default_rng(seed)
    out = []
    for i, m in enumerate(meshes):
        nv = np.asarray(m["pos"]).reshape(-1, 3).shape[0]
        slots = {UV1: rng.uniform(0, 1, (nv, 2)).astype(F), EX1: rng.uniform(-1, 1, (nv, 1)).astype(F),
                 EX2: rng.normal(size=(nv, 4)).astype(F), TAN: rng.normal(size=(nv, 3)).astype(F)}
        if i in skip_uv:
            del slots[UV1]
        out.append(dict(m, slots=slots))
    return out


def make_batch(meshes):
    rng = np.random.default_rng(7)
    pos = np.concatenate([np.asarray(m["pos"], F).reshape(-1, 3) for m in meshes]).astype(np.float64)
    lo, hi = pos.min(0), pos.max(0)
    c, ext = (lo + hi) / 2, float(np.linalg.norm(hi - lo))
    o = np.zeros((GROUPS, PER, 3), F)
    d = np.zeros((GROUPS, PER, 3), F)
    for g in range(GROUPS):
        u = rng.normal(size=3)
        u /= np.linalg.norm(u)
        eye = F(c + 0.9 * ext * u)
        targets = F(c + rng.uniform(-0.75, 0.75, (PER, 3)) * (hi - lo))
        o[g] = eye
        d[g] = targets - eye
    return o.reshape(-1, 3), d.reshape(-1, 3) + F(0.0)


def small_meshes(seed=5, counts=(5, 7), nv=9):
    """A few indexed meshes of random triangles around z = 1 (shared vertices, some -0.0 data)."""
    rng = np.random.default_rng(seed)
    out = []
    for c in counts:
        pos = rng.uniform(-1, 1, (nv, 3)).astype(F)
        pos[:, 2] += F(1.0)
        nrm = rng.normal(size=(nv, 3)).astype(F)
        idx = np.stack([rng.permutation(nv)[:3] for _ in range(c)]).astype(np.uint32).reshape(-1) if c else \
            np.zeros(0, np.uint32)
        out.append({"pos": pos, "nrm": nrm, "idx": idx})
    return out


_SUZ = {}


def suz(ctx):
    """Suzanne with synthetic slots, its GPU scene, the traced batch and the expected rows — made once."""
    if not _SUZ:
        meshes = with_slots(scenes.load_mesh("suzanne"), 2024)
        scene, keep = build(ctx, meshes)
        o, d = make_batch(meshes)
        res = scene.traceRays(o, d)
        hits = records(res["t"], res["u"], res["v"], res["tri_id"])
        exp = {r: expected(meshes, hits, *r) for r in SUZ_REQS}
        _SUZ["k"] = SimpleNamespace(meshes=meshes, scene=scene, keep=keep, o=o, d=d, hits=hits, exp=exp,
                                    hit=res["tri_id"] != np.uint32(NO_TRI))
    return _SUZ["k"]


def teardown_module(module):
    for k in _SUZ.values():
        k.scene.destroy()
    _SUZ.clear()


# ---- 1. Suzanne, traced hits -------------------------------------------------------------------------
def test_every_slot_at_traced_hits(ctx):
    k = suz(ctx)
    assert int(k.hit.sum()) >= 1000 and int((~k.hit).sum()) >= 1000, (int(k.hit.sum()), k.hit.size)
    reqs = [r for r in SUZ_REQS if not r[2]]
    assert {r[0] for r in reqs} == {UV1, EX1, EX2, TAN, POS, NRM, GEOM, FACE}
    for r, got in zip(reqs, query(k.scene, k.hits, reqs)):
        assert_rows(got, k.exp[r], f"request {r}")
        miss = got[~k.hit]
        if r[0] == FACE:
            assert got.dtype == np.int32 and np.all(miss == -1) and np.all(got[k.hit] >= 0)
        else:
            assert np.all(miss.view(np.uint32) == 0)  # +0.0 rows
            assert np.any(got[k.hit] != 0)


# ---- 2. NORMALIZE ------------------------------------------------------------------------------------
def test_normalize_matches_the_trace_primitives(ctx, oracle):
    k = suz(ctx)
    nn, gn, tn = query(k.scene, k.hits, [(NRM, 3, NORMALIZE), (GEOM, 3, NORMALIZE), (TAN, 3, NORMALIZE)])
    # z against orc_pin_ops out[10] on the same corner normals and (u, v), the record layout of bm_debug_primitives
    idx = np.flatnonzero(k.hit)
    g = k.hits.view(np.uint32)[idx, 3].astype(np.int64)
    mesh_of, face_of = mapping(k.meshes)
    rec = np.zeros((idx.size, 36), F)
    rec[:, 5] = 1.0
    rec[:, 6:15] = scenes.IDENTITY
    for i, m in enumerate(k.meshes):
        sel = np.flatnonzero(mesh_of[g] == i)
        iv = np.asarray(m["idx"]).reshape(-1, 3).astype(np.int64)[face_of[g[sel]]]
        rec[sel, 15:24] = np.asarray(m["pos"], F).reshape(-1, 3)[iv].reshape(-1, 9)
        rec[sel, 24:33] = np.asarray(m["nrm"], F).reshape(-1, 3)[iv].reshape(-1, 9)
    rec[:, 33], rec[:, 34] = k.hits[idx, 1], k.hits[idx, 2]
    fn = oracle.lib.orc_pin_ops
    fn.argtypes = [C.c_uint32, C.POINTER(C.c_float), C.POINTER(C.c_float)]
    fn.restype = None
    out = np.zeros((idx.size, 12), F)
    fn(idx.size, rec.ctypes.data_as(C.POINTER(C.c_float)), out.ctypes.data_as(C.POINTER(C.c_float)))
    assert np.array_equal(bits(nn[idx, 2]), bits(out[:, 10]))
    # x and y (and z again) against numpy with the same 1/sqrt; the geometric normal and a free slot likewise
    assert_rows(nn, k.exp[(NRM, 3, NORMALIZE)], "normal")
    assert_rows(gn, k.exp[(GEOM, 3, NORMALIZE)], "geometric normal")
    assert_rows(tn, k.exp[(TAN, 3, NORMALIZE)], "tangent")
    with np.errstate(all="ignore"):
        ln = np.sqrt((gn[idx].astype(np.float64) ** 2).sum(1))
    assert np.all(np.abs(ln - 1.0) < 1e-6)
    assert np.all(nn[~k.hit].view(np.uint32) == 0) and np.all(gn[~k.hit].view(np.uint32) == 0)


# ---- 3. hand-made hit records ------------------------------------------------------------------------
def corner_records(meshes):
    ntri = sum(np.asarray(m["idx"]).size // 3 for m in meshes)
    uv = F([[0, 0], [1, 0], [0, 1], [0.3125, 0.4375]])
    tri = np.repeat(np.arange(ntri, dtype=np.uint32), 4)
    u, v = np.tile(uv[:, 0], ntri), np.tile(uv[:, 1], ntri)
    return records(np.ones(tri.size, F), u, v, tri)


def test_hand_made_records_and_corners(ctx):
    meshes = with_slots(small_meshes(), 31)
    meshes[0]["slots"][EX1][::2] = F(-0.0)  # a corner may give +0 where the vertex holds -0
    meshes[1]["slots"][TAN][1] = F([-0.0, 0.0, -0.0])
    scene, keep = build(ctx, meshes)
    hits = corner_records(meshes)
    reqs = [(UV1, 2), (EX1, 1), (EX2, 4), (TAN, 3), (POS, 3), (NRM, 3), (GEOM, 3), (FACE, 2)]
    got = query(scene, hits, reqs)
    for r, a in zip(reqs, got):
        assert_rows(a, expected(meshes, hits, *r), f"request {r}")
    mesh_of, face_of = mapping(meshes)
    g = hits.view(np.uint32)[:, 3].astype(np.int64)
    for r, a in zip(reqs[:6], got[:6]):  # at corner c the vertex's own value, compared by value
        for i, m in enumerate(meshes):
            data = slot_data(m, r[0])
            iv = np.asarray(m["idx"]).reshape(-1, 3).astype(np.int64)
            for c in range(3):
                sel = np.flatnonzero((mesh_of[g] == i) & (np.arange(g.size) % 4 == c))
                assert sel.size == iv.shape[0]
                assert np.all(a[sel] == data[iv[face_of[g[sel]], c]]), (r, i, c)
    scene.destroy()


# ---- 4. many meshes ----------------------------------------------------------------------------------
def test_many_meshes_with_empty_ones_and_missing_slots(ctx):
    rng = np.random.default_rng(70)
    counts = [0 if i in (0, 33, 69) else int(rng.integers(1, 6)) for i in range(70)]
    no_uv = set(range(2, 70, 3))
    meshes = with_slots(small_meshes(seed=71, counts=counts, nv=7), 72, skip_uv=no_uv)
    scene, keep = build(ctx, meshes)
    mesh_of, face_of = mapping(meshes)
    first = np.concatenate([[0], np.cumsum(counts)[:-1]])
    ends = [(int(first[i]), int(first[i]) + c - 1) for i, c in enumerate(counts) if c]
    tri = np.uint32([t for pair in ends for t in pair])
    rng2 = np.random.default_rng(73)
    u = rng2.uniform(0, 0.5, tri.size).astype(F)
    v = rng2.uniform(0, 0.5, tri.size).astype(F)
    hits = records(np.ones(tri.size, F), u, v, tri)
    face, uv, ex2, pos = query(scene, hits, [(FACE, 2), (UV1, 2), (EX2, 4), (POS, 3)])
    host = np.array([[i, f] for i, c in enumerate(counts) for f in ((0, c - 1) if c else ())], np.int32)
    assert np.array_equal(face, host) and np.array_equal(face, expected(meshes, hits, FACE, 2))
    assert set(face[:, 0]) == set(range(70)) - {0, 33, 69}
    lacking = np.isin(face[:, 0], sorted(no_uv))
    assert lacking.any() and np.all(uv[lacking].view(np.uint32) == 0) and np.all(uv[~lacking] != 0)
    assert_rows(uv, expected(meshes, hits, UV1, 2), "uv1")
    assert_rows(ex2, expected(meshes, hits, EX2, 4), "extra2")
    assert_rows(pos, expected(meshes, hits, POS, 3), "position")
    # a slot no mesh has; then one mesh with a 3-component UV1 against the 2-component request
    with pytest.raises(beam.BeamError) as e:
        scene.hitAttributes(hits, [(EX4, 2)])
    assert e.value.code == FORMAT
    nv = meshes[4]["pos"].shape[0]
    assert 4 not in no_uv and counts[4] > 0
    assert keep[4].setVertexData(np.zeros((nv, 3), F), nv, 3, UV1) == 0
    with pytest.raises(beam.BeamError) as e:
        scene.hitAttributes(hits, [(UV1, 2)])
    assert e.value.code == FORMAT
    with pytest.raises(beam.BeamError) as e:  # ... and the other way round
        scene.hitAttributes(hits, [(UV1, 3)])
    assert e.value.code == FORMAT
    assert keep[4].setVertexData(meshes[4]["slots"][UV1], nv, 2, UV1) == 0
    assert_rows(scene.hitAttributes(hits, [(UV1, 2)])[0], expected(meshes, hits, UV1, 2), "uv1 again")
    scene.destroy()


# ---- 5. batch edges ----------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 63, 64, 65, 257])
def test_batch_edges_write_nothing_past_n(ctx, n):
    import torch
    k = suz(ctx)
    dev = torch.device("cuda", ctx.device)
    sel = np.concatenate([np.flatnonzero(k.hit)[:(n + 1) // 2], np.flatnonzero(~k.hit)[:n // 2]])
    sel.sort()
    h = np.full((n + 16, 4), -7.5, F)  # 64 sentinel words behind the records
    h[:n] = k.hits[sel]
    hits = torch.from_numpy(h).to(dev)
    out3 = torch.full((3 * n + 64,), -7.5, dtype=torch.float32, device=dev)
    out1 = torch.full((n + 64,), -7.5, dtype=torch.float32, device=dev)
    torch.cuda.synchronize()
    assert k.scene.hitAttributesDevice(hits.data_ptr(), n, [(NRM, 3, 0, out3.data_ptr()),
                                                             (EX1, 1, 0, out1.data_ptr())]) == 0
    ctx.sync()
    a3, a1, hb = out3.cpu().numpy(), out1.cpu().numpy(), hits.cpu().numpy()
    assert np.all(a3[3 * n:] == F(-7.5)) and np.all(a1[n:] == F(-7.5))
    assert np.array_equal(hb.view(np.uint32), h.view(np.uint32))
    assert_rows(a3[:3 * n].reshape(n, 3), k.exp[(NRM, 3, 0)][sel], "normal")
    assert_rows(a1[:n].reshape(n, 1), k.exp[(EX1, 1, 0)][sel], "extra1")


def test_out_of_range_ids_are_misses(ctx):
    k = suz(ctx)
    ntri = mapping(k.meshes)[0].size
    tri = np.uint32([ntri - 1, ntri, 0x7FFFFFFF, 0xFFFFFFFE, NO_TRI, 0])
    hits = records(np.ones(6, F), F([0.25] * 6), F([0.5] * 6), tri)
    hits[2, 1], hits[3, 2] = np.nan, np.inf  # u and v of a miss are not used either
    reqs = [(NRM, 3, NORMALIZE), (EX2, 4), (GEOM, 3), (FACE, 2)]
    live = np.array([True, False, False, False, False, True])
    for r, got in zip(reqs, query(k.scene, hits, reqs)):
        assert_rows(got, expected(k.meshes, hits, *r), f"request {r}")
        fill = -1 if r[0] == FACE else 0
        assert np.all(got[~live] == fill) and np.all(np.any(got[live] != fill, axis=1))


def test_non_finite_barycentrics_propagate(ctx):
    k = suz(ctx)
    hits = records(np.ones(3, F), F([np.inf, 0.25, np.nan]), F([0.25, -np.inf, 0.5]), np.uint32([3, 4, 5]))
    got, = k.scene.hitAttributes(hits, [(EX1, 1)])
    assert not np.isfinite(got).any()
    face, = k.scene.hitAttributes(hits, [(FACE, 2)])
    assert np.array_equal(face, expected(k.meshes, hits, FACE, 2))


# ---- 6. fused equals separate ------------------------------------------------------------------------
def test_one_fused_call_equals_four_calls(ctx):
    k = suz(ctx)
    reqs = [(POS, 3), (NRM, 3, NORMALIZE), (UV1, 2), (GEOM, 3)]
    fused = k.scene.hitAttributes(k.hits, reqs)
    for r, a in zip(reqs, fused):
        b, = k.scene.hitAttributes(k.hits, [r])
        assert a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32)), r
    mixed = k.scene.hitAttributes(k.hits, [(FACE, 2), (EX2, 4), (EX1, 1), (TAN, 3, NORMALIZE)])
    for r, a in zip([(FACE, 2, 0), (EX2, 4, 0), (EX1, 1, 0), (TAN, 3, NORMALIZE)], mixed):
        assert_rows(a, k.exp[r], f"request {r}")


# ---- 7. current buffers ------------------------------------------------------------------------------
def test_current_buffers_and_build_match(ctx):
    meshes = with_slots(small_meshes(seed=9), 32)
    scene, keep = build(ctx, meshes)
    hits = corner_records(meshes)
    check(scene, meshes, hits, [(UV1, 2), (POS, 3), (GEOM, 3)])
    # UV1 re-uploaded after the build: seen without a rebuild
    nv = meshes[1]["pos"].shape[0]
    new_uv = np.random.default_rng(33).uniform(2, 3, (nv, 2)).astype(F)
    assert keep[1].setVertexData(new_uv, nv, 2, UV1) == 0
    meshes[1]["slots"][UV1] = new_uv
    got, = scene.hitAttributes(hits, [(UV1, 2)])
    assert_rows(got, expected(meshes, hits, UV1, 2), "re-uploaded uv1")
    assert np.any(got > 2)
    # positions moved + refit: POSITION and GEOM_NORMAL follow
    before = scene.hitAttributes(hits, [(GEOM, 3)])[0]
    for i, m in enumerate(meshes):
        q = (m["pos"] * F(1.25) + F([0.5, -0.25, 0.125])).astype(F)
        q[:, 0] += F(0.3) * np.sin(m["pos"][:, 1]).astype(F)
        assert keep[i].setVertexData(q, q.shape[0], 3, POS) == 0
        meshes[i] = dict(m, pos=q)
    scene.refitGPUScene()
    check(scene, meshes, hits, [(POS, 3), (GEOM, 3), (GEOM, 3, NORMALIZE), (UV1, 2)])
    assert not np.array_equal(before, scene.hitAttributes(hits, [(GEOM, 3)])[0])
    # the same triangle count but an index beyond the vertices
    idx = np.asarray(meshes[0]["idx"], np.uint32)
    bad_idx = idx.copy()
    bad_idx[4] = nv
    assert keep[0].setIndices(bad_idx, bad_idx.size) == 0
    with pytest.raises(beam.BeamError) as e:
        scene.hitAttributes(hits, [(POS, 3)])
    assert e.value.code == BAD
    assert keep[0].setIndices(idx, idx.size) == 0
    check(scene, meshes, hits, [(POS, 3)])
    # a triangle count that is not the build's, then a mesh removed: no current build for this call
    assert keep[0].setIndices(idx[:-3], idx.size - 3) == 0
    with pytest.raises(beam.BeamError) as e:
        scene.hitAttributes(hits, [(POS, 3)])
    assert e.value.code == NOT_BUILT
    assert keep[0].setIndices(idx, idx.size) == 0
    check(scene, meshes, hits, [(POS, 3)])
    scene.removeMesh(keep[1])
    with pytest.raises(beam.BeamError) as e:
        scene.hitAttributes(hits, [(POS, 3)])
    assert e.value.code == NOT_BUILT
    scene.destroy()


# ---- 8. error table ----------------------------------------------------------------------------------
def test_errors(ctx):
    import torch
    k = suz(ctx)
    dev = torch.device("cuda", ctx.device)
    n = 64
    hits = torch.from_numpy(np.ascontiguousarray(k.hits[:n + 1])).to(dev)
    out = torch.zeros((n + 1, 4), dtype=torch.float32, device=dev)
    torch.cuda.synchronize()
    hp, op = hits.data_ptr(), out.data_ptr()
    s = k.scene
    call = s.hitAttributesDevice
    assert call(hp, n, [(NRM, 3, 0, op)]) == 0
    assert call(0, n, [(NRM, 3, 0, op)]) == BAD and call(hp, n, [(NRM, 3, 0, 0)]) == BAD  # null pointers, n > 0
    assert call(hp, n, [(NRM, 3, 0, op), (UV1, 2, 0, 0)]) == BAD
    assert call(hp + 4, n, [(NRM, 3, 0, op)]) == BAD and call(hp, n, [(NRM, 3, 0, op + 4)]) == BAD  # misaligned
    assert call(hp + 8, n, [(NRM, 3, 0, op)]) == BAD and call(hp, n, [(EX1, 1, 0, op + 8)]) == BAD
    assert call(hp, n, []) == BAD and call(hp, n, [(EX1, 1, 0, op)] * 5) == BAD  # 0 or more than 4 requests
    assert ctx.lib.bm_scene_hit_attributes(s.h, C.c_void_p(hp), n, None, 1) == BAD
    for slot in (10, 15, 18, 0xFFFFFFFF):  # unknown slots
        assert call(hp, n, [(slot, 3, 0, op)]) == BAD, slot
    for flags in (2, 3, 0x80000000):  # unknown flag bits
        assert call(hp, n, [(NRM, 3, flags, op)]) == BAD, flags
    for comps in (0, 5, 0xFFFFFFFF):
        assert call(hp, n, [(EX2, comps, 0, op)]) == BAD, comps
    for comps in (1, 2, 4):
        assert call(hp, n, [(GEOM, comps, 0, op)]) == BAD, comps
    for comps in (1, 3, 4):
        assert call(hp, n, [(FACE, comps, 0, op)]) == BAD, comps
    assert call(hp, n, [(UV1, 2, NORMALIZE, op)]) == BAD and call(hp, n, [(EX2, 4, NORMALIZE, op)]) == BAD
    assert call(hp, n, [(EX1, 1, NORMALIZE, op)]) == BAD and call(hp, n, [(FACE, 2, NORMALIZE, op)]) == BAD
    assert call(hp, n, [(NRM, 3, 0, op, 1)]) == BAD  # pad
    assert call(hp, n, [(NRM, 3, 0, op), (FACE, 2, 0, op, 7)]) == BAD
    # n = 0: nothing to read or write
    assert call(0, 0, [(NRM, 3, 0, 0)]) == 0 and call(hp, 0, [(NRM, 3, NORMALIZE, op), (FACE, 2, 0, 0)]) == 0
    assert s.hitAttributes(np.zeros((0, 4), F), [(EX2, 4), (FACE, 2)])[1].shape == (0, 2)
    assert call(hp, n, [(NRM, 3, 0, op)]) == 0
    ctx.sync()
    unbuilt = beam.IScene.create(ctx)
    assert unbuilt.hitAttributesDevice(hp, n, [(NRM, 3, 0, op)]) == NOT_BUILT
    assert unbuilt.hitAttributesDevice(0, 0, [(NRM, 3, 0, 0)]) == NOT_BUILT
    unbuilt.destroy()
    tiny = [{"pos": F([[0, 0, 1], [1, 0, 1], [0, 1, 1]]), "nrm": F([[0, 0, 1]] * 3), "idx": np.uint32([0, 1, 2])}]
    for kw in ({"reference_kd": True}, {"reference_hash": True}, {"bvh_width": 2}):
        other = beam.Context(device=0, **kw)
        sc, keep = build(other, tiny)
        assert sc.hitAttributesDevice(hp, n, [(NRM, 3, 0, op)]) == BAD, kw
        sc.destroy()
        other.close()


def test_empty_built_scene_has_only_misses(ctx):
    scene, keep = build(ctx, [])
    hits = records(np.ones(3, F), F([0.25] * 3), F([0.5] * 3), np.uint32([0, 7, NO_TRI]))
    ex, face = scene.hitAttributes(hits, [(EX4, 3), (FACE, 2)])
    assert np.all(ex.view(np.uint32) == 0) and np.all(face == -1)
    scene.destroy()


# ---- 9. OBJ end to end -------------------------------------------------------------------------------
def write_obj(path):
    """A 3 x 2 grid of quads over [-1.5, 1.5] x [-1, 1] around z = 1 in two material runs, with a bent surface,
    its normals and a sheared texture map."""
    xs, ys = np.linspace(-1.5, 1.5, 4), np.linspace(-1.0, 1.0, 3)
    lines = ["# hit-attribute fixture"]
    for y in ys:
        for x in xs:
            z = 1.0 + 0.1 * x * x + 0.05 * y
            lines.append(f"v {x:.6f} {y:.6f} {z:.6f}")
    for y in ys:
        for x in xs:
            lines.append(f"vt {0.5 + 0.3 * x + 0.05 * y:.6f} {0.5 + 0.4 * y - 0.1 * x:.6f}")
    for y in ys:
        for x in xs:
            nrm = np.array([0.2 * x, 0.05, -1.0])
            nrm /= np.linalg.norm(nrm)
            lines.append(f"vn {nrm[0]:.6f} {nrm[1]:.6f} {nrm[2]:.6f}")
    for row, mtl in ((0, "lower"), (1, "upper")):
        lines.append(f"usemtl {mtl}")
        for col in range(3):
            a = row * 4 + col + 1
            quad = (a, a + 1, a + 5, a + 4)
            lines.append("f " + " ".join(f"{i}/{i}/{i}" for i in quad))
    path.write_text("\n".join(lines) + "\n")


def test_obj_end_to_end(ctx, tmp_path):
    path = tmp_path / "grid.obj"
    write_obj(path)
    scene = beam.IScene.create(ctx)
    model = beam.Model.load(ctx, str(path), scene)
    scene.updateGPUScene()
    host = model.meshes()
    assert len(host) == 2 and all(m["idx"].size == 18 for m in host)
    meshes = []
    for m in host:
        assert m["uv"] is not None and m["tan"] is not None and m["bit"] is not None
        assert np.isfinite(m["tan"]).all() and np.isfinite(m["bit"]).all() and np.any(m["tan"] != 0)
        meshes.append({"pos": m["pos"], "nrm": m["nrm"], "idx": m["idx"],
                       "slots": {UV1: m["uv"], TAN: m["tan"], BIT: m["bit"]}})
    rng = np.random.default_rng(90)
    xy = rng.uniform([-1.4, -0.9], [1.4, 0.9], (24, 2))
    o = F(np.column_stack([xy, np.full(24, -1.0)]))
    d = np.tile(F([0.02, -0.01, 1.0]), (24, 1))
    res = scene.traceRays(o, d)
    assert np.all(res["tri_id"] != np.uint32(NO_TRI))
    hits = records(res["t"], res["u"], res["v"], res["tri_id"])
    face, = scene.hitAttributes(hits, [(FACE, 2)])
    assert set(face[:, 0]) == {0, 1}  # both material runs are hit
    check(scene, meshes, hits, [(UV1, 2), (TAN, 3), (BIT, 3), (NRM, 3, NORMALIZE)])
    check(scene, meshes, hits, [(POS, 3), (TAN, 3, NORMALIZE), (GEOM, 3), (FACE, 2)])
    scene.destroy()
    model.destroy()


# ---- 10. torch ---------------------------------------------------------------------------------------
def test_torch_chain_stays_on_the_device(ctx):
    import torch
    k = suz(ctx)
    dev = torch.device("cuda", 0)
    tctx = beam.Context(device=0, stream=torch.cuda.current_stream(dev).cuda_stream)
    scene, keep = build(tctx, k.meshes)
    n = k.o.shape[0]
    packed = np.zeros((n, 8), F)
    packed[:, 0:3], packed[:, 3], packed[:, 4:7] = k.o, np.inf, k.d
    rays = torch.from_numpy(packed).to(dev)
    # no synchronisation from here to the end of the chain
    res = scene.traceRays(rays)
    pos, nrm, face = scene.hitAttributes(res["hits"], [(POS, 3), (NRM, 3, NORMALIZE), (FACE, 2)])
    assert pos.is_cuda and pos.shape == (n, 3) and pos.dtype == torch.float32
    assert face.is_cuda and face.shape == (n, 2) and face.dtype == torch.int32
    hit = (res["tri_id"] >= 0)[:, None]
    lift = nrm * 0.001
    o2 = torch.where(hit, pos + lift, rays[:, 0:3])
    d2 = torch.where(hit, nrm, rays[:, 4:7])
    res2 = scene.traceRays(o2.contiguous(), d2.contiguous())
    torch.cuda.synchronize()
    # the same steps one by one through numpy on the module's scene
    assert np.array_equal(res["hits"].cpu().numpy().view(np.uint32), k.hits.view(np.uint32))
    assert_rows(pos.cpu().numpy(), k.exp[(POS, 3, 0)], "position")
    assert_rows(nrm.cpu().numpy(), k.exp[(NRM, 3, NORMALIZE)], "normal")
    assert np.array_equal(face.cpu().numpy(), k.exp[(FACE, 2, 0)])
    h = k.hit[:, None]
    lift_np = k.exp[(NRM, 3, NORMALIZE)] * F(0.001)
    o2_np = np.where(h, k.exp[(POS, 3, 0)] + lift_np, k.o).astype(F)
    d2_np = np.where(h, k.exp[(NRM, 3, NORMALIZE)], k.d).astype(F)
    assert np.array_equal(bits(o2.cpu().numpy()), bits(o2_np)) and np.array_equal(bits(d2.cpu().numpy()), bits(d2_np))
    step = k.scene.traceRays(o2_np, d2_np)
    got = res2["hits"].cpu().numpy()
    assert np.array_equal(got.view(np.uint32), records(step["t"], step["u"], step["v"], step["tri_id"]).view(np.uint32))
    assert np.any(step["tri_id"][k.hit] != np.uint32(NO_TRI))  # some bounce rays hit the model again
    scene.destroy()
    tctx.close()


# ---- 11. repeated-device context ---------------------------------------------------------------------
def test_rehearsal_context_queries_on_the_root(ctx):
    k = suz(ctx)
    multi = beam.Context(devices=[0, 0])
    scene, keep = build(multi, k.meshes)
    reqs = [(UV1, 2, 0), (NRM, 3, NORMALIZE), (GEOM, 3, 0), (FACE, 2, 0)]
    for r, got in zip(reqs, scene.hitAttributes(k.hits, reqs)):
        assert_rows(got, k.exp[r], f"request {r}")
    scene.destroy()
    multi.close()
