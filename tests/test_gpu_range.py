"""Every trace path on the range grid of tests/range_scenes.py: far eyes, large world offsets, tiny and huge
scales, four eye directions.

On every view, inside and outside the envelope (range_scenes.inside), the GPU equals the oracle's BVH trace bit
for bit: ids, packed colours, t, the traversal counters and, with the light, the shadow plane and the shadow
counters. The far views are where the paths have arithmetic that depends on the eye and that no other test
reaches: the compacted variant's cull margin (2^-12 of the larger of |eye| and the boxes) and its fast ray
set-up, the packet kernel's sign-sorted slab planes and its fork on a non-finite reciprocal, and the choice of
the kernel from the scene's coverage of the frame. Inside the envelope the frame also equals brute force
(tests/test_oracle_range.py checks the oracle's BVH against it on the whole grid, without a GPU).

The GPU side traces a part of the grid: D in {3, D_OK, 4096}, every offset, and the scales 2^-30, 2^30 (the
ends of the envelope), 2^44 (some triangle tests overflow) and 2^60 (all do: every pixel is a miss, since a
candidate whose t is +inf is no hit): 120 scene-views, about 30 s. FULL_GRID_SECONDS records what the whole
grid of 276 took, once, with no view differing; most of either time is the oracle's BVH answers on the CPU.

A test collects every view that differs and names them all when it fails.

The packet variant: wave packets visit subtrees in their first lane's order, and a ray's closest hit is
independent of that order only while the prune tn <= tbest is conservative, that is inside the envelope. The
library launches packets for eyes within BM_ENVELOPE_EXTENTS = D_OK extents of the scene and the quad kernel
beyond; the test checks which kernel ran (packets on every view up to D_OK, quads at 4096) and that the frame
equals the oracle's on all of them.

The automatic choice is traced at 192 x 192 with a light: it can come to quads or to cull+quads there. The
packet branch of that choice needs half a million covered pixels and no light
(tests/test_gpu_00_configs.py); no frame of this file reaches it.

test_the_cull_margin_follows_the_eye: at 32,768 extents |eye| is the only term of k_cull's margin that
covers the rounding of its slab distances; without it the cull drops rays whose exact traversal visits the
root, and the node counters fall short of the oracle's.
"""
from types import SimpleNamespace

import numpy as np
import pytest

import range_scenes as rs
from raytracercuda_amd import beam
from test_gpu_rays import MISS, assert_hits, oracle_anyhit, oracle_closest

pytestmark = pytest.mark.gpu

PRIO12, QUAD, COMPACT, PACKET = 6, 10, 12, 14
# every product path of tests/test_gpu_variants.py, BVH2 and both shadow modes (the variants' shadows are fused)
PATHS = {"single-lane": {"params": {"trace_variant": PRIO12}},
         "quad-dynamic": {"params": {"trace_variant": QUAD, "trace_sched": 1}},
         "quad-costorder": {"params": {"trace_variant": QUAD, "trace_sched": 2}},
         "compact-dynamic": {"params": {"trace_variant": COMPACT, "trace_sched": 1}},
         "packet": {"params": {"trace_variant": PACKET}},
         "bvh2": {"bvh_width": 2},
         "queued-shadows": {"shadow_queue": True}}
LEGAL_KINDS = ("quads", "cull+quads")  # what the automatic choice can come to at 192 x 192 with a light
FULL_GRID_SECONDS = 47  # every path and the automatic choice on all 276 scene-views; 28 s of it the oracle's answers
GPU_D, GPU_S = (3, rs.D_OK, 4096), (-30, 30, 44, 60)


def traced(v):
    return (v.T == 0 and v.s_exp == 0 and v.D in GPU_D) or v.T != 0 or v.s_exp in GPU_S


CASES = [(s, v) for s in rs.SCENES for v in rs.views_of(s) if traced(v)]
# brute force on the GPU side: every inside view of the two 3,000-triangle scenes, suzanne's at D_OK and T = 1e5
BRUTE = [(s, v) for s, v in CASES if rs.inside(v) and (s != "suzanne" or v.D == rs.D_OK or v.T == 1e5)]


@pytest.fixture(scope="module")
def answers(oracle):
    rs.warm(oracle, CASES, widths=(4, 2), brute=False)
    rs.warm(oracle, BRUTE)
    yield oracle
    rs.clear()


def placements(scene):
    """{(T, s_exp): views} of a scene: one GPU build each."""
    out = {}
    for s, v in CASES:
        if s == scene:
            out.setdefault((v.T, v.s_exp), []).append(v)
    return out


def build(ctx, meshes):
    scene = beam.IScene.create(ctx)
    keep = beam.upload_meshes(ctx, scene, meshes)
    scene.updateGPUScene()
    return scene, keep


def diff(f, cnt, e):
    """The planes and counters of a GPU frame that differ from the expected ones, as text ('' when none)."""
    bad = []
    for k, want in e.frame.items():
        if k not in f:
            continue
        got = f[k].view(np.uint32) if f[k].dtype == np.float32 else f[k]
        want = want.view(np.uint32) if want.dtype == np.float32 else want
        if not np.array_equal(got, want):
            at = np.flatnonzero(got != want)
            bad.append(f"{k}: {at.size} pixels, first at {at[:3].tolist()} got {got[at[:3]].tolist()} "
                       f"want {want[at[:3]].tolist()}")
    if cnt is not None and list(map(int, cnt)) != list(map(int, e.cnt[:len(cnt)])):
        bad.append(f"counters {list(map(int, cnt))} != {list(map(int, e.cnt[:len(cnt)]))}")
    return ", ".join(bad)


def read(rt, shadow):
    f = {k: a.reshape(-1) for k, a in rt.read().items()}
    if shadow:
        f["shadow"] = rt.readShadow().reshape(-1)
    return f


def no_id_without_a_finite_t(f):
    hit = f["tri_id"] != MISS
    return bool(np.array_equal(hit, np.isfinite(f["t"]) & (f["t"] > 0)))


@pytest.mark.parametrize("scene_name", rs.SCENES)
@pytest.mark.parametrize("path", PATHS)
def test_every_path_equals_the_oracle_bvh_on_every_view(answers, path, scene_name):
    """Counting and plain kernels, without and with the light."""
    oracle, width = answers, PATHS[path].get("bvh_width", 4)
    ctx = beam.Context(device=0, **PATHS[path])
    cam = beam.ICamera.create(ctx)
    rt = beam.IRenderTarget.createOffscreen(ctx, rs.W, rs.H)
    bad, n = [], 0
    for (T, s_exp), views in placements(scene_name).items():
        scene, keep = build(ctx, rs.meshes_of(scene_name, T, s_exp))
        for v in views:
            e = rs.bvh_expected(oracle, scene_name, v, width)
            assert cam.setInitialRays(rs.W, rs.H, *rs.camera(v)) == 0
            runs = []
            cnt = cam.traceCounters(e.eye, e.orient, scene, rt)
            runs.append(("counting", read(rt, False), cnt))
            assert cam.trace(e.eye, e.orient, scene, rt) == 0
            runs.append(("plain", read(rt, False), None))
            if path == "packet" and rt.traceKind() != ("packets" if v.D <= rs.D_OK else "quads"):
                bad.append(f"{v.id}: ran {rt.traceKind()}")
            cnt = cam.traceShadowCounters(e.eye, e.orient, scene, rt, e.light)
            runs.append(("shadow counting", read(rt, True), cnt))
            assert cam.traceShadow(e.eye, e.orient, scene, rt, e.light) == 0
            runs.append(("shadow", read(rt, True), None))
            for what, f, c in runs:
                d = diff(f, c, e)
                if not no_id_without_a_finite_t(f):
                    d += " a triangle id with a non-finite t"
                if d:
                    bad.append(f"{v.id} {what}: {d}")
            n += 1
        scene.destroy()
        del keep
    rt.destroy()
    cam.destroy()
    ctx.close()
    print(f"{path}, {scene_name}: {n} views, 4 traces each, {len(bad)} differ")
    assert not bad, "\n".join(bad)


@pytest.mark.parametrize("scene_name", ["cube", "soup"])
def test_the_cull_margin_follows_the_eye(oracle, scene_name):
    """The compacted variant at 32,768 extents, where |eye| is the only term of k_cull's margin large enough
    to cover the rounding of its own slab distances (about 1e-7 of |box - eye|)."""
    ctx = beam.Context(device=0, **PATHS["compact-dynamic"])
    cam = beam.ICamera.create(ctx)
    rt = beam.IRenderTarget.createOffscreen(ctx, rs.W, rs.H)
    scene, keep = build(ctx, rs.meshes_of(scene_name))
    bad = []
    for v in rs.VIEWS:
        if v.D != 32768:
            continue
        e = rs.bvh_expected(oracle, scene_name, v, 4)
        assert (e.frame["tri_id"] != MISS).mean() >= 0.25
        assert cam.setInitialRays(rs.W, rs.H, *rs.camera(v)) == 0
        cnt = cam.traceShadowCounters(e.eye, e.orient, scene, rt, e.light)
        d = diff(read(rt, True), cnt, e)
        assert cam.trace(e.eye, e.orient, scene, rt) == 0
        assert rt.traceKind() == "cull+quads"
        d += diff(read(rt, False), None, e)
        if d:
            bad.append(f"{v.id}: {d}")
    scene.destroy()
    del keep
    rt.destroy()
    cam.destroy()
    ctx.close()
    assert not bad, "\n".join(bad)


@pytest.mark.parametrize("scene_name", rs.SCENES)
def test_the_automatic_choice_on_a_target_stream_and_brute_force_inside_the_envelope(answers, scene_name):
    """The default context picks its kernel per frame from the scene's coverage of the frame (quads or, on a
    target with a stream of its own as frames in flight use, cull+quads for a sparse view; see the module
    docstring for the packet branch). Inside the envelope the same frame equals brute force."""
    import torch
    oracle = answers
    ctx = beam.Context(device=0)
    cam = beam.ICamera.create(ctx)
    rt = beam.IRenderTarget.createOffscreen(ctx, rs.W, rs.H)
    stream = torch.cuda.Stream()
    rt.setStream(stream.cuda_stream)
    brute_views = {v.id for s, v in BRUTE if s == scene_name}
    bad, kinds = [], {}
    for (T, s_exp), views in placements(scene_name).items():
        scene, keep = build(ctx, rs.meshes_of(scene_name, T, s_exp))
        for v in views:
            e = rs.bvh_expected(oracle, scene_name, v, 4)
            assert cam.setInitialRays(rs.W, rs.H, *rs.camera(v)) == 0
            assert cam.traceShadow(e.eye, e.orient, scene, rt, e.light) == 0
            f = read(rt, True)
            kind = rt.traceKind()
            kinds[kind] = kinds.get(kind, 0) + 1
            d = diff(f, None, e)
            if kind not in LEGAL_KINDS:
                d += f" trace kind {kind!r}"
            if v.id in brute_views:
                b = SimpleNamespace(frame=rs.brute_expected(oracle, scene_name, v), cnt=None)
                db = diff(f, None, b)
                d += f" against brute force: {db}" if db else ""
            if d:
                bad.append(f"{v.id}: {d}")
        scene.destroy()
        del keep
    rt.destroy()
    cam.destroy()
    ctx.close()
    print(f"automatic choice, {scene_name}: kinds {kinds}; {len(brute_views)} views against brute force")
    assert len(brute_views) >= 8
    assert not bad, "\n".join(bad)


# ---- ray queries ---------------------------------------------------------------------------------------
ORIGINS, PER = 16, 61
QUERY_PLACEMENTS = [(1e5, 0), (0.0, 44)]


def query_batch(scene_name, T, s_exp):
    """16 origins at 3, D_OK and 4096 extents in turn, in random directions; 61 rays each to targets in the
    scene's box. The any-hit segments run to twice the target's distance; the oracle takes a segment's end
    point and forms end - origin itself, which is the direction the GPU is given."""
    rng = np.random.default_rng(77)
    o = np.zeros((ORIGINS, PER, 3), np.float32)
    d = np.zeros((ORIGINS, PER, 3), np.float32)
    for g in range(ORIGINS):
        u = rng.normal(size=3)
        u /= np.linalg.norm(u)
        o[g] = rs.place(GPU_D[g % 3] * u, T, s_exp)
        d[g] = rs.place(rng.uniform(-0.6, 0.6, (PER, 3)), T, s_exp) - o[g]
    o, d = o.reshape(-1, 3), d.reshape(-1, 3) + np.float32(0.0)
    end = o + (d + d)
    return o, d, end, end - o


@pytest.mark.parametrize("placement", QUERY_PLACEMENTS, ids=["T1e5", "S2^44"])
@pytest.mark.parametrize("scene_name", rs.SCENES)
def test_ray_queries_far_away_and_at_a_huge_scale(ctx, oracle, scene_name, placement):
    T, s_exp = placement
    meshes = rs.meshes_of(scene_name, T, s_exp)
    obvh = rs.oracle_bvh(oracle, scene_name, T, s_exp, 4)
    o, d, end, sd = query_batch(scene_name, T, s_exp)
    exp, cnt = oracle_closest(oracle, obvh, meshes, o, d, per=PER)
    hit = exp["tri_id"] != MISS
    assert 0.1 <= hit.mean() <= 0.95 and np.all(np.isfinite(exp["t"][hit])), float(hit.mean())
    scene, keep = build(ctx, meshes)
    res = scene.traceRays(o, d, counters=True)
    assert np.all(np.isfinite(res["t"][res["tri_id"] != MISS])) and np.all(np.isposinf(res["t"][res["tri_id"] == MISS]))
    assert_hits(res, exp)
    assert list(map(int, res["counters"])) == list(map(int, cnt)), (res["counters"], cnt)
    assert_hits(scene.traceRays(o, d), exp)  # the non-counting kernel
    occ, ocnt = oracle_anyhit(obvh, o, end)
    assert 0 < occ.sum() < occ.size
    got = scene.traceRays(o, sd, any_hit=True, counters=True)
    assert np.array_equal(got["occluded"], occ), int((got["occluded"] != occ).sum())
    assert list(map(int, got["counters"])) == list(map(int, ocnt)), (got["counters"], ocnt)
    print(f"{scene_name} T {T:g} S 2^{s_exp}: {int(hit.sum())} of {hit.size} rays hit, {int(occ.sum())} of "
          f"{occ.size} segments occluded")
    scene.destroy()
    del keep


# ---- refit and instances -------------------------------------------------------------------------------
@pytest.mark.parametrize("scene_name", rs.SCENES)
def test_refit_to_a_far_offset_pads_for_the_new_coordinates(ctx, answers, scene_name):
    """Built at the origin, every vertex moved by 1e5 extents, refit: the records are orc_bvh_refit's, and the
    frame equals the rebuilt oracle's and brute force (another tree, the same closest hits)."""
    oracle = answers
    v = rs.BY_ID[rs.view_id(SimpleNamespace(D=3, dir="diag", T=1e5, s_exp=0))]
    base, moved = rs.meshes_of(scene_name), rs.meshes_of(scene_name, 1e5, 0)
    scene = beam.IScene.create(ctx)
    gm = beam.upload_meshes(ctx, scene, base)
    scene.updateGPUScene(stats=True)
    for m, mv in zip(gm, moved):
        assert m.setVertexData(mv["pos"], mv["pos"].shape[0], 3, beam.VERTEX_DATA_POSITION) == 0
    scene.refitGPUScene()
    rec, tris, _, _ = scene.export()
    orec, otris, _, _ = oracle.bvh_build(base, 4, 4).refit(moved).export()
    reach = beam.reachable_records(orec)
    assert np.array_equal(tris, otris) and np.array_equal(rec[reach], orec[reach])
    e = rs.bvh_expected(oracle, scene_name, v, 4)
    cam = beam.ICamera.create(ctx)
    assert cam.setInitialRays(rs.W, rs.H, *rs.camera(v)) == 0
    rt = beam.IRenderTarget.createOffscreen(ctx, rs.W, rs.H)
    assert cam.traceShadow(e.eye, e.orient, scene, rt, e.light) == 0
    f = read(rt, True)
    assert not diff(f, None, e), diff(f, None, e)
    b = SimpleNamespace(frame=rs.brute_expected(oracle, scene_name, v), cnt=None)
    assert not diff(f, None, b), diff(f, None, b)
    rt.destroy()
    cam.destroy()
    scene.destroy()


@pytest.mark.parametrize("scene_name", ["cube", "soup"])
def test_an_instance_placed_far_and_large_equals_the_baked_mesh(ctx, oracle, scene_name):
    """One instance by a 3x4 matrix of scale 2^10 and translation 1e5 * OFFSET against the mesh transformed on
    the host (tests/test_instances_abi.py's float32 restatement), the oracle's BVH and brute force on it."""
    from test_gpu_instances import instanced, plain, pretransformed
    v = SimpleNamespace(D=3, dir="oblique", T=1e5, s_exp=10)
    x = np.concatenate([np.eye(3) * 2.0 ** 10, (1e5 * rs.OFFSET)[:, None]], axis=1).astype(np.float32)
    entries = [(m, x) for m in rs.meshes_of(scene_name)]
    a, keep_a, _ = instanced(ctx, entries)
    b, keep_b, _ = plain(ctx, entries)
    baked = pretransformed(entries)
    eye, orient, light = rs.eye_of(v), rs.orient_of(v), rs.light_of(v)
    rays = rs.rays_of(oracle, v)
    obvh = oracle.bvh_build(baked, 4, 4)
    packed, tri, t = obvh.render(rays, eye, orient)
    want = {"packed": packed, "tri_id": tri, "t": t, "shadow": obvh.shadow(rays, eye, orient, light, tri, t)}
    bp, btri, bt = oracle.brute_render(baked, rays, eye, orient)
    brute = {"packed": bp, "tri_id": btri, "t": bt, "shadow": oracle.brute_shadow(baked, rays, eye, orient, light, btri, bt)}
    assert 0.25 <= (tri != MISS).mean() <= 0.9
    cam = beam.ICamera.create(ctx)
    assert cam.setInitialRays(rs.W, rs.H, *rs.camera(v)) == 0
    rt = beam.IRenderTarget.createOffscreen(ctx, rs.W, rs.H)
    for scene in (a, b):
        assert cam.traceShadow(eye, orient, scene, rt, light) == 0
        f = read(rt, True)
        for ref in (want, brute):
            d = diff(f, None, SimpleNamespace(frame=ref, cnt=None))
            assert not d, d
    rt.destroy()
    cam.destroy()
    a.destroy()
    b.destroy()
