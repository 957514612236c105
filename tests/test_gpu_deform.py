"""GPU checks of device-side mesh deformation: bm_mesh_compute_normals against its numpy restatement bit for bit,
device uploads and read-backs (bm_mesh_set_vertex_data_device, bm_mesh_copy_vertex_data_device), and the loop
"upload, normals, refit, query" against the same loop through the host path.

No expected value comes from the code under test: normals are tests/test_deform_abi.py's vertex_normals (the
header's definition in numpy float32, one rounding per statement), and the loop's comparison scene gets its
positions and those normals through bm_mesh_set_vertex_data, which this feature does not touch.
"""
import ctypes as C

import numpy as np
import pytest

from gpu_util import gpu_frame
from raytracercuda_amd import _lib, beam, scenes
from test_deform_abi import corner_table, vertex_normals

pytestmark = pytest.mark.gpu

F = np.float32
POS, NRM, UV1, TAN, EX1, EX2 = (beam.VERTEX_DATA_POSITION, beam.VERTEX_DATA_NORMAL, beam.VERTEX_DATA_UV1,
                                beam.VERTEX_DATA_TANGENT, beam.VERTEX_DATA_EXTRA1, beam.VERTEX_DATA_EXTRA2)
BAD, NO_VERTS, FORMAT = _lib.ERROR_INVALID_PARAMETER, _lib.ERROR_NO_VERTICES, _lib.ERROR_INVALID_FORMAT
W = H = 256
EYE = (0.0, 0.0, -4.0)
SHIFT = F([1000, -2000, 500])


def dev0():
    import torch
    return torch.device("cuda", 0)


def to_dev(a):
    """A numpy array as a torch tensor on the device, its upload finished (the context stream reads it)."""
    import torch
    t = torch.from_numpy(np.ascontiguousarray(a)).to(dev0())
    torch.cuda.current_stream(dev0()).synchronize()
    return t


def bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


def assert_bits(got, exp, what="", nan_as_nan=False):
    """Bit images; nan_as_nan: a NaN matches a NaN (its sign and payload are the processor's, not the contract's)."""
    got, exp = np.asarray(got), np.asarray(exp)
    assert got.shape == exp.shape and got.dtype == exp.dtype == F, (what, got.shape, exp.shape, got.dtype)
    same = bits(got) == bits(exp)
    if nan_as_nan:
        same |= np.isnan(got) & np.isnan(exp)
    assert same.all(), f"{what}: {int((~same.all(axis=-1)).sum())} of {got.shape[0]} rows differ"


def make_mesh(ctx, pos, idx=None, nrm=None):
    m = beam.IMesh.create(ctx)
    pos = np.asarray(pos, F).reshape(-1, 3)
    if idx is not None and np.asarray(idx).size:
        i = np.ascontiguousarray(idx, np.uint32).reshape(-1)
        ctx._check(m.setIndices(i, i.size))
    ctx._check(m.setVertexData(pos, pos.shape[0], 3, POS))
    if nrm is not None:
        ctx._check(m.setVertexData(np.asarray(nrm, F), pos.shape[0], 3, NRM))
    return m


def read_slot(ctx, mesh, slot):
    t = mesh.vertexData(slot)
    ctx.sync()
    return t.cpu().numpy()


def gpu_normals(ctx, mesh, normalize):
    mesh.computeNormals(normalize)
    return read_slot(ctx, mesh, NRM)


def check_normals(ctx, pos, idx, what, nan_as_nan=False):
    """Both forms of bm_mesh_compute_normals on a fresh mesh against the restatement, and a second call."""
    mesh = make_mesh(ctx, pos, idx)
    flat = np.zeros(0, np.uint32) if idx is None else np.asarray(idx, np.uint32).reshape(-1)
    for normalize in (True, False):
        exp = vertex_normals(pos, flat, normalize)
        assert_bits(gpu_normals(ctx, mesh, normalize), exp, f"{what}, normalize={normalize}", nan_as_nan)
    assert_bits(gpu_normals(ctx, mesh, True), vertex_normals(pos, flat, True), f"{what}, again", nan_as_nan)
    mesh.destroy()


# ---- meshes ------------------------------------------------------------------------------------------
def strip(nv, seed=3):
    """nv vertices along a noisy ribbon, the nv - 2 triangles of their strip with alternating winding."""
    rng = np.random.default_rng(seed + nv)
    k = np.arange(nv)
    pos = np.stack([k * 0.5, (k % 2) * 1.0, np.sin(k * 0.7)], axis=1) + rng.normal(0, 0.1, (nv, 3))
    tri = [(i, i + 1, i + 2) if i % 2 == 0 else (i + 1, i, i + 2) for i in range(max(nv - 2, 0))]
    return F(pos), np.array(tri, np.uint32).reshape(-1)


def fan(valence, seed=5):
    """Vertex 0 in the middle of `valence` triangles (0, i, i + 1) over a noisy spiral of valence + 1 rim
    vertices."""
    rng = np.random.default_rng(seed + valence)
    a = np.arange(valence + 1) * (2 * np.pi / max(valence, 6))
    rim = np.stack([np.cos(a), np.sin(a), 0.2 * np.sin(3 * a)], axis=1) + rng.normal(0, 0.02, (valence + 1, 3))
    pos = np.concatenate([[[0.0, 0.0, 0.5]], rim])
    tri = [(0, i, i + 1) for i in range(1, valence + 1)]
    return F(pos), np.array(tri, np.uint32).reshape(-1)


def suzanne():
    m, = scenes.load_mesh("suzanne")
    return np.asarray(m["pos"], F).reshape(-1, 3), np.asarray(m["idx"], np.uint32).reshape(-1)


def displaced(pos, step):
    """The positions moved by a smooth field that depends on the step: float32, computed on the host."""
    p = np.asarray(pos, F)
    return (p + F(0.06) * np.sin(F(3.0 + step) * p[:, [1, 2, 0]] + F(0.7 * step))).astype(F)


# ---- 1. normals: bit images against the restatement ------------------------------------------------------
def test_one_triangle_and_two_sharing_an_edge(ctx):
    check_normals(ctx, F([[0, 0, 0], [2, 0, 0.5], [0.25, 3, 0]]), [0, 1, 2], "one triangle")
    check_normals(ctx, F([[0, 0, 0], [2, 0, 0.5], [0.25, 3, 0], [2.5, 2.75, -1]]), [0, 1, 2, 2, 1, 3], "two triangles")


@pytest.mark.parametrize("nv", [1, 3, 4, 5, 63, 64, 65, 255, 256, 257])
def test_strips_meet_every_tail_of_the_launch(ctx, nv):
    pos, idx = strip(nv)
    assert pos.shape[0] == nv and idx.size == 3 * max(nv - 2, 0)
    check_normals(ctx, pos, idx, f"strip of {nv}")


@pytest.mark.parametrize("valence", [1, 2, 63, 64, 65, 300])
def test_fans(ctx, valence):
    pos, idx = fan(valence)
    assert np.count_nonzero(idx == 0) == valence
    check_normals(ctx, pos, idx, f"fan of {valence}")


def test_unnamed_vertex_degenerate_face_and_a_vertex_named_twice(ctx):
    pos = F([[0, 0, 0], [1, 0, 0], [0, 1, 0], [5, 5, 5], [2, 0, 0], [0.5, 0.25, 1]])
    # vertex 3 is in no face; (0, 1, 4) is collinear: zero area; (5, 5, 2) names vertex 5 twice
    idx = [0, 1, 2, 0, 1, 4, 5, 5, 2, 2, 1, 5]
    check_normals(ctx, pos, idx, "special cases")
    exp = vertex_normals(pos, idx)
    assert not exp[3].any() and not exp[4].any() and exp[5].any()
    # only degenerate faces anywhere: all zeros, no NaN
    check_normals(ctx, pos, [0, 1, 4, 5, 5, 2], "degenerate only")
    assert not vertex_normals(pos, [0, 1, 4, 5, 5, 2]).any()


def test_mesh_without_indices_gets_zeros(ctx):
    pos, _ = strip(70)
    mesh = make_mesh(ctx, pos)
    for normalize in (True, False):
        got = gpu_normals(ctx, mesh, normalize)
        assert got.shape == (70, 3) and not got.view(np.uint32).any()
    mesh.destroy()


def test_non_finite_values_follow_the_arithmetic(ctx):
    pos = F([[0, 0, 0], [1e10, 0, 0], [0, 1e10, 0], [np.nan, 0, 0], [0, 1, 0], [1, 1, 1]])
    idx = [0, 1, 2, 3, 4, 5]  # s.z = 1e20 with d = +inf: zeros; a NaN position: NaN
    exp = vertex_normals(pos, idx)
    assert not exp[:3].any() and np.isnan(exp[3:]).any(axis=1).all()
    check_normals(ctx, pos, idx, "non-finite", nan_as_nan=True)


@pytest.mark.parametrize("name", ["suzanne", "bunny", "suzanne moved"])
def test_fixture_meshes(ctx, name):
    m, = scenes.load_mesh(name.split()[0])
    pos, idx = np.asarray(m["pos"], F).reshape(-1, 3), np.asarray(m["idx"], np.uint32).reshape(-1)
    if name.endswith("moved"):
        pos = pos + SHIFT
    if name.startswith("suzanne"):
        assert pos.shape[0] == 7830
    check_normals(ctx, pos, idx, name)


@pytest.mark.parametrize("nv", [5, 64, 257])
def test_nothing_is_written_behind_the_last_vertex(ctx, nv):
    """The kernel over the test's own buffers (bm_debug_vertex_normals) and the restatement's table: the rows
    are the restatement's, the sentinel row behind them is untouched."""
    pos, idx = strip(nv)
    offsets, corners = corner_table(idx, nv)
    table = np.concatenate([offsets, corners]).astype(np.uint32)
    d_pos, d_idx, d_tab = to_dev(pos), to_dev(idx.view(np.int32)), to_dev(table.view(np.int32))
    for normalize in (True, False):
        out = np.full((nv + 1, 3), F(-7.25), F)
        d_out = to_dev(out)
        ctx._check(ctx.lib.bm_debug_vertex_normals(ctx.h, d_pos.data_ptr(), d_idx.data_ptr(), d_tab.data_ptr(),
                                                   d_out.data_ptr(), nv, 1 if normalize else 0))
        ctx.sync()
        got = d_out.cpu().numpy()
        assert_bits(got[:nv], vertex_normals(pos, idx, normalize), f"rows of {nv}")
        assert_bits(got[nv:], out[nv:], "sentinel")


# ---- 2. the table ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("grid", [1, 2])
def test_trace_grid_does_not_touch_the_result(grid):
    pos, idx = suzanne()
    c = beam.Context(device=0, params={"trace_grid": grid})
    check_normals(c, pos, idx, f"trace_grid {grid}")
    c.close()


def test_new_indices_rebuild_the_table(ctx):
    pos, idx = fan(65)
    mesh = make_mesh(ctx, pos, idx)
    first = gpu_normals(ctx, mesh, True)
    assert_bits(first, vertex_normals(pos, idx), "first topology")
    # the same vertices, other faces, fewer and in another order; then more faces than ever before
    idx2 = np.ascontiguousarray(idx.reshape(-1, 3)[::-2, [1, 2, 0]]).reshape(-1)
    idx3 = np.concatenate([idx, idx2, idx.reshape(-1, 3)[:, [0, 2, 1]].reshape(-1)])
    for k, new in enumerate((idx2, idx3, idx)):
        ctx._check(mesh.setIndices(new, new.size))
        exp = vertex_normals(pos, new)
        assert_bits(gpu_normals(ctx, mesh, True), exp, f"topology {k}")
        assert_bits(gpu_normals(ctx, mesh, False), vertex_normals(pos, new, False), f"topology {k}, raw")
    assert (bits(vertex_normals(pos, idx2)) != bits(first)).any()
    mesh.destroy()


# ---- 3. device uploads -----------------------------------------------------------------------------------
def test_upload_and_read_back_every_component_count(ctx):
    rng = np.random.default_rng(11)
    nv = 257
    pos, idx = strip(nv)
    mesh = make_mesh(ctx, pos, idx)
    data = {}
    for slot, comp in ((UV1, 2), (EX1, 1), (EX2, 4), (TAN, 3), (POS, 3), (NRM, 3)):
        data[slot] = rng.normal(size=(nv, comp)).astype(F)
        data[slot].reshape(-1)[::7] = F(np.nan)  # any bit pattern goes through
        t = to_dev(data[slot] if slot != EX2 else data[slot].reshape(-1))  # flat is accepted too
        assert mesh.setVertexData(t, nv, comp, slot) == 0
    for slot, exp in data.items():  # after all uploads: no slot disturbed another
        got = read_slot(ctx, mesh, slot)
        assert got.shape == exp.shape
        assert np.array_equal(bits(got), bits(exp)), slot
    # the read-back is a copy: a later upload does not change a tensor read earlier
    early = mesh.vertexData(UV1)
    mesh.setVertexData(to_dev(np.zeros((nv, 2), F)), nv, 2, UV1)
    ctx.sync()
    assert np.array_equal(bits(early.cpu().numpy()), bits(data[UV1]))
    assert not read_slot(ctx, mesh, UV1).any()
    mesh.destroy()


def test_host_and_device_uploads_alternate(ctx):
    nv = 65
    pos, idx = strip(nv)
    mesh = make_mesh(ctx, pos, idx)
    for step in range(1, 5):
        p = displaced(pos, step)
        if step % 2:
            assert mesh.setVertexData(to_dev(p), nv, 3, POS) == 0
        else:
            assert mesh.setVertexData(p, nv, 3, POS) == 0
        assert np.array_equal(bits(read_slot(ctx, mesh, POS)), bits(p)), step
        assert_bits(gpu_normals(ctx, mesh, True), vertex_normals(p, idx), f"step {step}")
    mesh.destroy()


def test_bad_tensors_raise(ctx):
    import torch
    nv = 16
    pos, idx = strip(nv)
    mesh = make_mesh(ctx, pos, idx)
    good = to_dev(pos)
    bad = [(torch.from_numpy(pos), nv, 3),                        # on the host
           (good.to(torch.float64), nv, 3),                       # dtype
           (good.to(torch.float16), nv, 3),
           (good.t(), nv, 3),                                     # (3, nv): shape, and not contiguous
           (to_dev(np.zeros((nv, 4), F))[:, :3], nv, 3),          # a strided view
           (to_dev(np.zeros((nv + 1, 3), F)), nv, 3),             # more rows than numVertices
           (to_dev(np.zeros((nv, 2), F)), nv, 3),                 # other components
           (to_dev(np.zeros((nv + 1, 3), F)), nv + 1, 3),         # another vertex count than the mesh's
           (to_dev(np.zeros((nv, 2), F)), nv, 2)]                 # positions have 3 components
    for t, n, comp in bad:
        with pytest.raises(beam.BeamError) as e:
            mesh.setVertexData(t, n, comp, POS)
        assert e.value.code == BAD
    with pytest.raises(beam.BeamError) as e:
        mesh.setVertexData(to_dev(np.zeros((nv, 5), F)), nv, 5, UV1)
    assert e.value.code == BAD
    with pytest.raises(beam.BeamError) as e:
        mesh.setVertexData(good, nv, 3, beam.VERTEX_DATA_COUNT)
    assert e.value.code == BAD
    assert np.array_equal(bits(read_slot(ctx, mesh, POS)), bits(pos))  # nothing was written
    mesh.destroy()


# ---- 4. the loop -----------------------------------------------------------------------------------------
XFORM = np.array([[0.8, 0.0, 0.6, 0.3], [0.0, 1.0, 0.0, -0.2], [-0.6, 0.0, 0.8, 0.4]], F)


def loop_rays(n=1000, seed=17):
    rng = np.random.default_rng(seed)
    u = rng.normal(size=(n, 3))
    u /= np.linalg.norm(u, axis=1, keepdims=True)
    o = F(4.0 * u)
    d = F(rng.uniform(-1.0, 1.0, (n, 3))) - o
    return o, d


def hit_records(res):
    h = np.zeros((res["t"].shape[0], 4), F)
    h[:, 0], h[:, 1], h[:, 2] = res["t"], res["u"], res["v"]
    h.view(np.uint32)[:, 3] = res["tri_id"]
    return h


def add_entry(scene, mesh, instance):
    if instance:
        scene.addInstance(mesh, XFORM)
    else:
        scene.addMesh(mesh)


def assert_same_frame(fa, fb, what):
    assert {"packed", "tri_id", "t"} <= set(fa) and set(fa) == set(fb)
    for k in fa:
        assert np.array_equal(fa[k].view(np.uint32), fb[k].view(np.uint32)), (what, k)
    assert (fa["tri_id"] != beam.NO_TRIANGLE).sum() > 1000, what  # the model is in the picture


@pytest.mark.parametrize("kind", ["plain", "instance", "bvh2"])
def test_the_loop_equals_the_host_path(ctx, kind):
    pos, idx = suzanne()
    nv = pos.shape[0]
    own = beam.Context(device=0, bvh_width=2) if kind == "bvh2" else None
    c = own or ctx
    queries = kind != "bvh2"  # ray queries and hit attributes: BVH4 scenes only
    # scene A: everything through the host path; scene B: positions only, normals from the kernel
    mesh_a = make_mesh(c, pos, idx, vertex_normals(pos, idx))
    mesh_b = make_mesh(c, pos, idx)
    scene_a, scene_b = beam.IScene.create(c), beam.IScene.create(c)
    add_entry(scene_a, mesh_a, kind == "instance")
    add_entry(scene_b, mesh_b, kind == "instance")
    scene_a.updateGPUScene()
    with pytest.raises(beam.BeamError) as e:  # no normals yet
        scene_b.updateGPUScene()
    assert e.value.code == FORMAT
    mesh_b.computeNormals()
    scene_b.updateGPUScene()
    o, d = loop_rays()
    for step in range(4):  # the build, then three displacements by refit
        if step:
            p = displaced(pos, step)
            assert mesh_a.setVertexData(p, nv, 3, POS) == 0
            assert mesh_a.setVertexData(vertex_normals(p, idx), nv, 3, NRM) == 0
            scene_a.refitGPUScene()
            assert mesh_b.setVertexData(to_dev(p), nv, 3, POS) == 0
            mesh_b.computeNormals()
            scene_b.refitGPUScene()
        fa = gpu_frame(c, scene_a, W, H, scenes.RAYS_SQUARE, EYE, scenes.IDENTITY)
        fb = gpu_frame(c, scene_b, W, H, scenes.RAYS_SQUARE, EYE, scenes.IDENTITY)
        assert_same_frame(fa, fb, f"{kind}, step {step}")
        if queries:
            ra, rb = scene_a.traceRays(o, d), scene_b.traceRays(o, d)
            for k in ("t", "u", "v", "tri_id"):
                assert np.array_equal(ra[k].view(np.uint32), rb[k].view(np.uint32)), (kind, step, k)
            assert (ra["tri_id"] != beam.NO_TRIANGLE).sum() > 100
            hits = hit_records(ra)
            reqs = [(NRM, 3), (POS, 3), (NRM, 3, beam.ATTR_NORMALIZE)]
            for r, xa, xb in zip(reqs, scene_a.hitAttributes(hits, reqs), scene_b.hitAttributes(hits, reqs)):
                assert np.array_equal(bits(xa), bits(xb)), (kind, step, r)
    for x in (scene_a, scene_b, mesh_a, mesh_b):
        x.destroy()
    if own:
        own.close()


# ---- 5. ordering on one stream ---------------------------------------------------------------------------
def test_everything_is_ordered_on_torch_s_stream(ctx):
    import torch
    from test_gpu_attrs import expected
    pos, idx = suzanne()
    nv = pos.shape[0]
    dev = dev0()
    tctx = beam.Context(device=0, stream=torch.cuda.current_stream(dev).cuda_stream)
    mesh = make_mesh(tctx, pos, idx)
    mesh.computeNormals()
    scene = beam.IScene.create(tctx)
    scene.addMesh(mesh)
    scene.updateGPUScene()
    o, d = loop_rays()
    packed = np.zeros((o.shape[0], 8), F)
    packed[:, 0:3], packed[:, 3], packed[:, 4:7] = o, np.inf, d
    rays = to_dev(packed)
    p0 = to_dev(pos)
    mesh.computeNormals()  # the table is built: nothing below waits for the device
    torch.cuda.synchronize()
    # no synchronisation from here to the end of the chain
    p1 = p0 + 0.06 * torch.sin(4.0 * p0[:, [1, 2, 0]] + 0.7)
    mesh.setVertexData(p1, nv, 3, POS)
    mesh.computeNormals()
    scene.refitGPUScene()
    res = scene.traceRays(rays)
    before = scene.hitAttributes(res["hits"], [(POS, 3), (NRM, 3)])
    p2 = p0 + 0.09 * torch.cos(5.0 * p0[:, [2, 0, 1]])
    mesh.setVertexData(p2, nv, 3, POS)
    p1.zero_()  # the first upload's source, rewritten after the copy in stream order
    mesh.computeNormals()
    after = scene.hitAttributes(res["hits"], [(POS, 3), (NRM, 3)])
    torch.cuda.synchronize()
    # the same through the host path, on the session's context
    p1_np = (p0 + 0.06 * torch.sin(4.0 * p0[:, [1, 2, 0]] + 0.7)).cpu().numpy()
    p2_np = p2.cpu().numpy()
    assert (bits(p1_np) != bits(pos)).any() and (bits(p2_np) != bits(p1_np)).any()
    mesh_a = make_mesh(ctx, pos, idx, vertex_normals(pos, idx))
    scene_a = beam.IScene.create(ctx)
    scene_a.addMesh(mesh_a)
    scene_a.updateGPUScene()
    assert mesh_a.setVertexData(p1_np, nv, 3, POS) == 0
    scene_a.refitGPUScene()
    ra = scene_a.traceRays(o, d)
    hits = res["hits"].cpu().numpy()
    assert np.array_equal(hits.view(np.uint32), hit_records(ra).view(np.uint32))
    assert (ra["tri_id"] != beam.NO_TRIANGLE).sum() > 100
    for got, p, what in ((before, p1_np, "before the second upload"), (after, p2_np, "after it")):
        m = [{"pos": p, "nrm": vertex_normals(p, idx), "idx": idx}]
        assert_bits(got[0].cpu().numpy(), expected(m, hits, POS, 3), f"position {what}")
        assert_bits(got[1].cpu().numpy(), expected(m, hits, NRM, 3), f"normal {what}")
    for x in (scene, mesh, scene_a, mesh_a):
        x.destroy()
    tctx.close()


# ---- 6. errors, and the repeated-device context ------------------------------------------------------------
def test_error_table(ctx):
    lib = ctx.lib
    nv = 8
    pos, idx = strip(nv)
    buf = to_dev(np.zeros((nv + 1, 4), F))
    ptr = buf.data_ptr()
    mesh = beam.IMesh.create(ctx)
    # an empty mesh
    assert lib.bm_mesh_compute_normals(mesh.h, 1) == NO_VERTS
    assert lib.bm_mesh_copy_vertex_data_device(mesh.h, POS, ptr, nv, 3) == NO_VERTS
    # bm_mesh_set_vertex_data_device: bm_mesh_set_vertex_data's table
    for args in ((None, nv, 3, POS), (ptr, 0, 3, POS), (ptr, nv, 3, beam.VERTEX_DATA_COUNT), (ptr, nv, 0, UV1),
                 (ptr, nv, 5, UV1), (ptr, nv, 2, POS), (ptr, nv, 4, POS)):
        assert lib.bm_mesh_set_vertex_data_device(mesh.h, *args) == BAD, args
        host = (C.c_float * (5 * (nv + 1)))()
        assert lib.bm_mesh_set_vertex_data(mesh.h, None if args[0] is None else host, *args[1:]) == BAD, args
    assert "setVertexData" in ctx.last_error()
    assert mesh.setVertexData(to_dev(pos), nv, 3, POS) == 0
    assert lib.bm_mesh_set_vertex_data_device(mesh.h, ptr, nv + 1, 2, UV1) == BAD  # another vertex count
    assert mesh.setVertexData(buf[:nv, :2].contiguous(), nv, 2, UV1) == 0
    ctx.sync()
    # bm_mesh_copy_vertex_data_device
    assert lib.bm_mesh_copy_vertex_data_device(mesh.h, POS, None, nv, 3) == BAD
    assert lib.bm_mesh_copy_vertex_data_device(mesh.h, beam.VERTEX_DATA_COUNT, ptr, nv, 3) == BAD
    assert lib.bm_mesh_copy_vertex_data_device(mesh.h, POS, ptr, nv + 1, 3) == BAD
    assert lib.bm_mesh_copy_vertex_data_device(mesh.h, POS, ptr, nv, 4) == BAD
    assert lib.bm_mesh_copy_vertex_data_device(mesh.h, UV1, ptr, nv, 3) == BAD
    assert lib.bm_mesh_copy_vertex_data_device(mesh.h, TAN, ptr, nv, 3) == NO_VERTS
    assert lib.bm_mesh_copy_vertex_data_device(mesh.h, UV1, ptr, nv, 2) == 0
    with pytest.raises(beam.BeamError) as e:
        mesh.vertexData(TAN)
    assert e.value.code == NO_VERTS
    with pytest.raises(beam.BeamError) as e:
        mesh.vertexData(beam.VERTEX_DATA_COUNT)
    assert e.value.code == BAD
    # bm_mesh_compute_normals
    for flags in (2, 3, 0x80000000):
        assert lib.bm_mesh_compute_normals(mesh.h, flags) == BAD
    big = idx.copy()
    big[-1] = nv  # an index at the vertex count
    ctx._check(mesh.setIndices(big, big.size))
    assert lib.bm_mesh_compute_normals(mesh.h, 1) == BAD
    assert "index out of range" in ctx.last_error()
    ctx._check(mesh.setIndices(idx, idx.size))
    assert_bits(gpu_normals(ctx, mesh, True), vertex_normals(pos, idx), "after the errors")
    # a mesh with a slot, but not positions
    other = beam.IMesh.create(ctx)
    assert lib.bm_mesh_set_vertex_data_device(other.h, ptr, nv, 2, UV1) == 0
    assert lib.bm_mesh_compute_normals(other.h, 1) == NO_VERTS
    other.destroy()
    mesh.destroy()


def test_repeated_device_context_replicas_follow(ctx):
    pos, idx = suzanne()
    nv = pos.shape[0]
    p = displaced(pos, 2)
    # the comparison: one device, host path
    mesh_a = make_mesh(ctx, pos, idx, vertex_normals(pos, idx))
    scene_a = beam.IScene.create(ctx)
    scene_a.addMesh(mesh_a)
    scene_a.updateGPUScene()
    assert mesh_a.setVertexData(p, nv, 3, POS) == 0
    assert mesh_a.setVertexData(vertex_normals(p, idx), nv, 3, NRM) == 0
    scene_a.refitGPUScene()
    fa = gpu_frame(ctx, scene_a, W, H, scenes.RAYS_SQUARE, EYE, scenes.IDENTITY)
    multi = beam.Context(devices=[0, 0])
    mesh = make_mesh(multi, pos, idx)
    mesh.computeNormals()
    scene = beam.IScene.create(multi)
    scene.addMesh(mesh)
    scene.updateGPUScene()
    assert mesh.setVertexData(to_dev(p), nv, 3, POS) == 0
    mesh.computeNormals()
    scene.refitGPUScene()
    fb = gpu_frame(multi, scene, W, H, scenes.RAYS_SQUARE, EYE, scenes.IDENTITY)  # bands from both replicas
    assert_same_frame(fa, fb, "devices=[0, 0]")
    assert_bits(read_slot(multi, mesh, NRM), vertex_normals(p, idx), "root normals")
    for x in (scene, mesh):
        x.destroy()
    multi.close()
    for x in (scene_a, mesh_a):
        x.destroy()
