"""GPU checks of instance transforms (bm_scene_add_instance, bm_scene_set_instance_transform + refit).

No expected value comes from the code under test. The meshes are pre-transformed on the host by the numpy
float32 restatement of the header's arithmetic (tests/test_instances_abi.py: one operation per statement) and
go through the existing bm_scene_add_mesh path and the existing oracle. The build is deterministic, so an
instanced scene and a plain scene of the pre-transformed meshes must agree bit for bit: export, frames, ray
queries and hit attributes.
"""
import numpy as np
import pytest

from gpu_util import assert_frame_equal, gpu_frame, oracle_frame
from raytracercuda_amd import _lib, beam, scenes
from test_gpu_attrs import NO_TRI, assert_rows, expected, records, with_slots, write_obj
from test_instances_abi import MIRROR, ROTATION, SCALE, rotation, xform_mesh

pytestmark = pytest.mark.gpu

F = np.float32
POS, NRM, UV1, TAN = beam.VERTEX_DATA_POSITION, beam.VERTEX_DATA_NORMAL, beam.VERTEX_DATA_UV1, beam.VERTEX_DATA_TANGENT
GEOM, FACE, NORMALIZE = beam.ATTR_GEOM_NORMAL, beam.ATTR_MESH_FACE, beam.ATTR_NORMALIZE
BAD = _lib.ERROR_INVALID_PARAMETER
W = H = 256
EYE = (0.0, 0.0, -7.0)


def placed(x, t):
    """The (3,4) transform x with its translation replaced."""
    out = np.array(x, F)
    out[:, 3] = F(t)
    return out


# Suzanne fits in [-1.4, 1.4]^3: the plain entry in the middle, three placements around it, all in view of EYE
T0 = [placed(ROTATION, (-2.6, 1.4, 1.0)), placed(SCALE, (2.2, -1.6, 0.5)), placed(MIRROR, (2.4, 1.5, 1.5))]
T1 = [placed(rotation((3, -1, 2), 1.9), (-2.2, -1.5, 0.25)), placed(SCALE * F(0.75), (2.5, 1.2, 2.0)),
      placed(rotation((0, 1, 0), 0.4) @ np.diag(F([1, 1, -1, 1])), (-2.4, 1.7, 3.0))]


def upload(ctx, scene, entries):
    """entries: (mesh dict, None) for a plain entry or (mesh dict, xform) for an instance; a dict seen twice is
    uploaded once. Returns the IMesh of every entry."""
    made, out = {}, []
    for m, x in entries:
        if id(m) not in made:
            tmp = beam.IScene.create(ctx)
            made[id(m)] = beam.upload_meshes(ctx, tmp, [m])[0]
            tmp.destroy()
        mesh = made[id(m)]
        if x is None:
            scene.addMesh(mesh)
        else:
            assert scene.addInstance(mesh, x) == len(out)
        out.append(mesh)
    return out


def instanced(ctx, entries):
    scene = beam.IScene.create(ctx)
    keep = upload(ctx, scene, entries)
    return scene, keep, scene.updateGPUScene(stats=True)


def pretransformed(entries):
    return [m if x is None else xform_mesh(x, m) for m, x in entries]


def plain(ctx, entries):
    """The comparison scene: the entries' meshes transformed on the host, each uploaded as a mesh of its own."""
    scene = beam.IScene.create(ctx)
    keep = beam.upload_meshes(ctx, scene, pretransformed(entries))
    return scene, keep, scene.updateGPUScene(stats=True)


def assert_same_build(a, b, sa=None, sb=None):
    ra, ta, ka, pa = a.export()
    rb, tb, kb, pb = b.export()
    assert np.array_equal(pa, pb), "perm"
    assert np.array_equal(ka, kb), "keys"
    assert np.array_equal(ta, tb), f"tris: {int((ta != tb).any(axis=1).sum())} of {ta.shape[0]} differ"
    assert ra.shape == rb.shape
    reach = beam.reachable_records(ra)
    assert np.array_equal(reach, beam.reachable_records(rb)) and np.array_equal(ra[reach], rb[reach]), "records"
    if sa is not None:
        assert sa["num_tris"] == sb["num_tris"] and sa["num_records"] == sb["num_records"]
        assert sa["num_meshes"] == sb["num_meshes"]


def frame(ctx, scene, w=W, h=H, rgb=True):
    return gpu_frame(ctx, scene, w, h, scenes.RAYS_SQUARE, EYE, scenes.IDENTITY, rgb=rgb)


def assert_same_frame(fa, fb):
    """Every plane read back, bit for bit."""
    assert set(fa) == set(fb) and {"packed", "tri_id", "t"} <= set(fa)
    for k in fa:
        assert np.array_equal(fa[k].view(np.uint32), fb[k].view(np.uint32)), k


def suz_entries(xforms, slots=False):
    base = scenes.load_mesh("suzanne")
    if slots:
        base = with_slots(base, 2024)
    return [(m, None) for m in base] + [(m, x) for x in xforms for m in base]


def ray_batch(lo, hi, groups=64, per=61, seed=7):
    """3,904 rays: per group one eye outside the box [lo, hi] and `per` targets in and around it."""
    rng = np.random.default_rng(seed)
    lo, hi = np.asarray(lo, np.float64), np.asarray(hi, np.float64)
    c, ext = (lo + hi) / 2, float(np.linalg.norm(hi - lo))
    o = np.zeros((groups, per, 3), F)
    d = np.zeros((groups, per, 3), F)
    for g in range(groups):
        u = rng.normal(size=3)
        u /= np.linalg.norm(u)
        eye = F(c + 0.9 * ext * u)
        o[g] = eye
        d[g] = F(c + rng.uniform(-0.75, 0.75, (per, 3)) * (hi - lo)) - eye
    return o.reshape(-1, 3), d.reshape(-1, 3) + F(0.0)


def box_of(meshes):
    pos = np.concatenate([np.asarray(m["pos"], F).reshape(-1, 3) for m in meshes])
    return pos.min(0), pos.max(0)


# ---- 1. export parity --------------------------------------------------------------------------------
def test_export_and_frame_parity_with_pretransformed_meshes(ctx, oracle):
    entries = suz_entries(T0)
    a, keep_a, sa = instanced(ctx, entries)
    b, keep_b, sb = plain(ctx, entries)
    assert sa["num_meshes"] == len(entries) and sa["num_tris"] > 0
    assert_same_build(a, b, sa, sb)
    fa, fb = frame(ctx, a), frame(ctx, b)
    assert_same_frame(fa, fb)
    pre = pretransformed(entries)
    packed, tri, t = oracle_frame(oracle, pre, W, H, scenes.RAYS_SQUARE, EYE, scenes.IDENTITY)
    assert_frame_equal(fa, packed, tri, t)
    # all four placements are in the picture
    counts = np.cumsum([0] + [np.asarray(m["idx"]).size // 3 for m in pre])
    hit_entries = set(np.searchsorted(counts, tri[tri != NO_TRI], side="right") - 1)
    assert hit_entries == set(range(len(entries)))
    a.destroy()
    b.destroy()


# ---- 2. unit and tail edges --------------------------------------------------------------------------
def synthetic(nv, rng, indexed=True):
    """nv vertices, every one referenced by a triangle (k-th triangle: vertices 3k, 3k+1, 3k+2 modulo nv)."""
    pos = rng.uniform(-1, 1, (nv, 3)).astype(F)
    nrm = rng.normal(size=(nv, 3)).astype(F)
    idx = (np.arange(3 * ((nv + 2) // 3)) % nv).astype(np.uint32) if indexed else np.zeros(0, np.uint32)
    return {"pos": pos, "nrm": nrm, "idx": idx}


def test_unit_and_tail_edges(ctx):
    rng = np.random.default_rng(41)
    sizes = [1, 3, 4, 5, 255, 256, 257, 1025]
    xf = [ROTATION, SCALE, MIRROR] + [placed(rotation(rng.normal(size=3), rng.uniform(0, 6)) * F(rng.uniform(0.5, 2)),
                                             rng.uniform(-2, 2, 3)) for _ in range(6)]
    entries = []
    for k, nv in enumerate(sizes):
        m = synthetic(nv, rng)
        assert set(m["idx"].tolist()) == set(range(nv))
        entries.append((m, xf[k]))
        if k % 2 == 0:
            entries.append((synthetic(6, rng), None))  # a plain entry in between
    entries.insert(5, (synthetic(7, rng, indexed=False), xf[8]))  # vertices, no triangles
    shared = entries[-1][0]
    entries.append((shared, xf[0]))  # the 1,025-vertex mesh a second time, elsewhere
    a, keep_a, sa = instanced(ctx, entries)
    b, keep_b, sb = plain(ctx, entries)
    assert sa["num_meshes"] == len(entries) == 14
    assert_same_build(a, b, sa, sb)
    a.destroy()
    b.destroy()


# ---- 3. many entries ---------------------------------------------------------------------------------
def test_many_entries_export_and_ray_queries(ctx):
    rng = np.random.default_rng(300)
    m = {"pos": rng.uniform(-0.4, 0.4, (5, 3)).astype(F), "nrm": rng.normal(size=(5, 3)).astype(F),
         "idx": np.uint32([0, 1, 2, 2, 3, 4, 4, 0, 1])}
    entries = [(m, placed(rotation(rng.normal(size=3), rng.uniform(0, 6)), rng.uniform(-3, 3, 3))) for _ in range(300)]
    a, keep_a, sa = instanced(ctx, entries)
    b, keep_b, sb = plain(ctx, entries)
    assert sa["num_meshes"] == 300 and sa["num_tris"] == 900
    assert_same_build(a, b, sa, sb)
    o, d = ray_batch(*box_of(pretransformed(entries)))
    assert o.shape[0] == 3904
    ra, rb = a.traceRays(o, d), b.traceRays(o, d)
    for k in ("t", "u", "v", "tri_id"):
        assert np.array_equal(ra[k].view(np.uint32), rb[k].view(np.uint32)), k
    hits = int((ra["tri_id"] != np.uint32(NO_TRI)).sum())
    assert 100 <= hits < 3904, hits
    oa, ob = a.traceRays(o, d, any_hit=True), b.traceRays(o, d, any_hit=True)
    assert np.array_equal(oa["occluded"], ob["occluded"]) and oa["occluded"].any()
    a.destroy()
    b.destroy()


# ---- 4. refit animation ------------------------------------------------------------------------------
def test_refit_animation(ctx, oracle):
    e0, e1 = suz_entries(T0), suz_entries(T1)
    per = len(e0) // (1 + len(T0))  # meshes of the model: entries 0..per-1 plain, then per entries per matrix
    a, keep_a, _ = instanced(ctx, e0)
    b, keep_b, _ = plain(ctx, e0)
    f0 = frame(ctx, a)
    for k, x in enumerate(T1):
        for j in range(per):
            a.setInstanceTransform(per * (1 + k) + j, x)
    # nothing moves before the refit; the matrix read back is the one just set, bit for bit
    assert_same_frame(frame(ctx, a), f0)
    for k, x in enumerate(T1):
        got = a.instanceTransform(per * (1 + k))
        assert got.shape == (3, 4) and np.array_equal(got.view(np.uint32), x.view(np.uint32))
    a.refitGPUScene()
    pre1 = pretransformed(e1)
    for mesh, m in zip(keep_b, pre1):
        assert mesh.setVertexData(m["pos"], m["pos"].shape[0], 3, POS) == 0
        assert mesh.setVertexData(m["nrm"], m["nrm"].shape[0], 3, NRM) == 0
    b.refitGPUScene()
    assert_same_build(a, b)
    f1 = frame(ctx, a)
    assert_same_frame(f1, frame(ctx, b))
    assert not np.array_equal(f1["tri_id"], f0["tri_id"])
    packed, tri, t = oracle_frame(oracle, pre1, W, H, scenes.RAYS_SQUARE, EYE, scenes.IDENTITY)
    assert_frame_equal(f1, packed, tri, t)
    # new positions for the base mesh + refit: the plain entry and every instance of it move
    base = [m for m, x in e1[:per]]
    moved = [dict(m, pos=(np.asarray(m["pos"], F) * F([1.0, 1.25, 0.75]) + F([0.0, 0.1, 0.0])).astype(F)) for m in base]
    for j in range(per):
        assert keep_a[j].setVertexData(moved[j]["pos"], moved[j]["pos"].shape[0], 3, POS) == 0
    a.refitGPUScene()
    e2 = [(m, None) for m in moved] + [(m, x) for x in T1 for m in moved]
    pre2 = pretransformed(e2)
    for mesh, m in zip(keep_b, pre2):
        assert mesh.setVertexData(m["pos"], m["pos"].shape[0], 3, POS) == 0
    b.refitGPUScene()
    assert_same_build(a, b)
    f2 = frame(ctx, a)
    assert_same_frame(f2, frame(ctx, b))
    assert not np.array_equal(f2["t"], f1["t"])
    a.destroy()
    b.destroy()


# ---- 5. hit attributes -------------------------------------------------------------------------------
def test_hit_attributes_world_space_and_as_uploaded(ctx):
    entries = suz_entries(T0, slots=True)
    a, keep_a, _ = instanced(ctx, entries)
    pre = pretransformed(entries)  # positions and normals transformed, the synthetic slots as uploaded
    assert all(np.array_equal(p["slots"][UV1], m["slots"][UV1]) for p, (m, x) in zip(pre, entries))
    o, d = ray_batch(*box_of(pre))
    res = a.traceRays(o, d)
    hits = records(res["t"], res["u"], res["v"], res["tri_id"])
    hit = res["tri_id"] != np.uint32(NO_TRI)
    assert int(hit.sum()) >= 500 and int((~hit).sum()) >= 100, int(hit.sum())
    reqs = [(POS, 3, 0), (NRM, 3, 0), (NRM, 3, NORMALIZE), (GEOM, 3, 0), (UV1, 2, 0), (TAN, 3, 0), (FACE, 2, 0)]
    single = {}
    for r in reqs:
        got, = a.hitAttributes(hits, [r])
        assert_rows(got, expected(pre, hits, *r), f"request {r}")
        single[r] = got
    face = single[(FACE, 2, 0)]
    counts = np.cumsum([0] + [np.asarray(m["idx"]).size // 3 for m in pre])
    entry_of = np.searchsorted(counts, res["tri_id"][hit].astype(np.int64), side="right") - 1
    assert np.array_equal(face[hit, 0], entry_of) and set(entry_of) == set(range(len(entries)))
    fused_reqs = [(POS, 3, 0), (NRM, 3, NORMALIZE), (UV1, 2, 0), (GEOM, 3, 0)]
    for r, got in zip(fused_reqs, a.hitAttributes(hits, fused_reqs)):
        assert np.array_equal(got.view(np.uint32), single[r].view(np.uint32)), r
    # A mesh cannot grow: every slot shares the vertex count of the first upload (setVertexData refuses another
    # count), so an instance's pool regions can never be shorter than its mesh. Indices past the vertices are the
    # existing error; within them the call keeps working.
    mesh, m = keep_a[-1], entries[-1][0]
    nv = np.asarray(m["pos"]).reshape(-1, 3).shape[0]
    grown = np.concatenate([np.asarray(m["pos"], F).reshape(-1, 3), np.zeros((3, 3), F)])
    assert mesh.setVertexData(grown, nv + 3, 3, POS) == BAD
    idx = np.asarray(m["idx"], np.uint32)
    past = idx.copy()
    past[-1] = nv
    assert mesh.setIndices(past, past.size) == 0
    with pytest.raises(beam.BeamError) as e:
        a.hitAttributes(hits, [(POS, 3)])
    assert e.value.code == BAD
    with pytest.raises(beam.BeamError):
        a.refitGPUScene()
    assert mesh.setIndices(idx, idx.size) == 0
    a.refitGPUScene()
    assert_rows(a.hitAttributes(hits, [(POS, 3)])[0], single[(POS, 3, 0)], "position after the refit")
    a.destroy()


# ---- 6. other modes ----------------------------------------------------------------------------------
@pytest.mark.parametrize("kw", [{"reference_kd": True}, {"reference_hash": True}, {"bvh_width": 2}],
                         ids=["reference_kd", "reference_hash", "bvh2"])
def test_other_modes_equal_their_pretransformed_scene(kw):
    entries = suz_entries(T0)
    lo, hi = box_of(pretransformed(entries))
    assert lo.min() > -30.0 and hi.max() < 30.0  # inside the reference's world box
    other = beam.Context(device=0, **kw)
    a, keep_a, _ = instanced(other, entries)
    fa = frame(other, a, 128, 128, rgb=False)
    a.destroy()
    b, keep_b, _ = plain(other, entries)
    fb = frame(other, b, 128, 128, rgb=False)
    b.destroy()
    assert_same_frame(fa, fb)
    assert int((fa["tri_id"] != np.uint32(NO_TRI)).sum()) > 500
    other.close()


def test_repeated_device_context_equals_single_device(ctx):
    entries = suz_entries(T0)
    a, keep_a, _ = instanced(ctx, entries)
    ref = frame(ctx, a)
    a.destroy()
    multi = beam.Context(devices=[0, 0])
    m, keep_m, _ = instanced(multi, entries)
    assert_same_frame(frame(multi, m), ref)
    per = len(entries) // (1 + len(T0))
    for k, x in enumerate(T1):  # the replicas follow set + refit
        for j in range(per):
            m.setInstanceTransform(per * (1 + k) + j, x)
    m.refitGPUScene()
    s, keep_s, _ = instanced(ctx, suz_entries(T1))
    assert_same_frame(frame(multi, m), frame(ctx, s))
    s.destroy()
    m.destroy()
    multi.close()


# ---- 7. entry bookkeeping and errors -----------------------------------------------------------------
def tri_mesh(z):
    return {"pos": F([[-1, -1, z], [1, -1, z], [0, 1, z]]), "nrm": F([[0, 0, -1]] * 3), "idx": np.uint32([0, 1, 2])}


def test_entry_bookkeeping_and_errors(ctx, tmp_path):
    ident = np.concatenate([np.eye(3), np.zeros((3, 1))], axis=1).astype(F)
    scene = beam.IScene.create(ctx)
    st = scene.updateGPUScene(stats=True)  # zero entries build as before
    assert st["num_tris"] == 0 and st["num_meshes"] == 0
    tmp = beam.IScene.create(ctx)
    m0, m1, m2 = beam.upload_meshes(ctx, tmp, [tri_mesh(1.0), tri_mesh(2.0), tri_mesh(3.0)])
    tmp.destroy()
    xa, xb, xc = placed(ident, (0, 0, 1)), placed(ident, (0, 0, 2)), placed(SCALE, (1, 0, 0))
    scene.addMesh(m0)                           # 0 plain
    assert scene.addInstance(m1, xa) == 1       # 1
    assert scene.addInstance(m1, xb.reshape(12)) == 2
    scene.addMesh(m2)                           # 3 plain
    four = np.concatenate([xc, F([[0, 0, 0, 1]])])
    assert scene.addInstance(m0, four) == 4
    with pytest.raises(beam.BeamError) as e:    # unbuilt after adds: refit fails as for addMesh
        scene.refitGPUScene()
    assert e.value.code == BAD
    scene.updateGPUScene()
    assert np.array_equal(scene.instanceTransform(4), xc)
    # rejected: a plain entry, an index past the list, non-finite elements, a mesh of another context
    for index in (0, 3, 5, 0xFFFFFFFF):
        with pytest.raises(beam.BeamError) as e:
            scene.setInstanceTransform(index, xa)
        assert e.value.code == BAD, index
        with pytest.raises(beam.BeamError) as e:
            scene.instanceTransform(index)
        assert e.value.code == BAD, index
    for bad_value in (np.nan, np.inf, -np.inf):
        for k in (0, 7, 11):
            x = xa.copy().reshape(12)
            x[k] = bad_value
            with pytest.raises(beam.BeamError) as e:
                scene.setInstanceTransform(1, x)
            assert e.value.code == BAD
            with pytest.raises(beam.BeamError) as e:
                scene.addInstance(m0, x)
            assert e.value.code == BAD
    assert np.array_equal(scene.instanceTransform(1), xa)  # a rejected matrix changes nothing
    with pytest.raises(beam.BeamError) as e:
        scene.removeInstance(5)
    assert e.value.code == BAD
    other = beam.Context(device=0)
    foreign = beam.IMesh.create(other)
    with pytest.raises(beam.BeamError) as e:
        scene.addInstance(foreign, xa)
    assert e.value.code == BAD
    foreign.destroy()
    other.close()
    scene.refitGPUScene()  # none of the rejected calls marked the scene unbuilt
    # a singular matrix is accepted
    flat = np.array([[1, 0, 0, 0], [0, 1, 0, 0], [0, 0, 0, 1]], F)
    scene.setInstanceTransform(2, flat)
    scene.refitGPUScene()
    scene.setInstanceTransform(2, xb)
    # removeInstance(1): the later entries move down by one; removeMesh(m1) then takes the first entry of m1
    scene.removeInstance(1)
    with pytest.raises(beam.BeamError) as e:    # unbuilt after a removal
        scene.refitGPUScene()
    assert e.value.code == BAD
    assert np.array_equal(scene.instanceTransform(1), xb) and np.array_equal(scene.instanceTransform(3), xc)
    with pytest.raises(beam.BeamError):
        scene.instanceTransform(2)              # now the plain entry of m2
    scene.removeMesh(m1)                        # entries: m0 plain, m2 plain, m0 at xc
    assert np.array_equal(scene.instanceTransform(2), xc)
    with pytest.raises(beam.BeamError):
        scene.instanceTransform(1)
    scene.removeInstance(0)                     # a plain entry by index: m2 plain, m0 at xc
    assert np.array_equal(scene.instanceTransform(1), xc)
    st = scene.updateGPUScene(stats=True)
    assert st["num_meshes"] == 2 and st["num_tris"] == 2
    cmp_scene, keep, _ = plain(ctx, [(tri_mesh(3.0), None), (tri_mesh(1.0), xc)])
    assert_same_build(scene, cmp_scene)
    two = records(np.ones(2, F), F([0.25, 0.25]), F([0.25, 0.25]), np.uint32([0, 1]))
    face, = scene.hitAttributes(two, [(FACE, 2)])
    assert np.array_equal(face, np.int32([[0, 0], [1, 0]]))
    cmp_scene.destroy()
    scene.destroy()
    # Model.addInstance on a two-material OBJ equals adding its meshes by hand
    path = tmp_path / "grid.obj"
    write_obj(path)
    x = placed(ROTATION, (0.5, 0.25, 2.0))
    sa = beam.IScene.create(ctx)
    model = beam.Model(str(path))
    model.addInstance(ctx, sa, x)
    model.addInstance(ctx, sa, xa)  # uploaded once, added again
    sta = sa.updateGPUScene(stats=True)
    assert sta["num_meshes"] == 4 and sta["num_tris"] == 24
    sb = beam.IScene.create(ctx)
    by_hand = beam.Model(str(path))
    by_hand.upload(ctx)
    for xf in (x, xa):
        for i in range(2):
            xx = np.ascontiguousarray(xf, F).reshape(12)
            ctx._check(ctx.lib.bm_scene_add_instance(sb.h, by_hand.gpu_mesh(i), beam._fp(xx), None))
    stb = sb.updateGPUScene(stats=True)
    assert_same_build(sa, sb, sta, stb)
    host = [{"pos": m["pos"], "nrm": m["nrm"], "idx": m["idx"]} for m in model.meshes()]
    sc, keep_c, stc = plain(ctx, [(m, xf) for xf in (x, xa) for m in host])
    assert_same_build(sa, sc, sta, stc)
    for s in (sa, sb, sc):
        s.destroy()
    model.destroy()
    by_hand.destroy()
